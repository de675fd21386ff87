"""GPU, two devices in one process: the launchers keep their dynamic-LDS limits and device queries per device
(mmego_amd/csrc/launch_setup.h), so the same seeded work run on cuda:0 and then on cuda:1 gives bit-identical results.  Skips itself
where fewer than two devices are visible."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _split3_forward_and_ul_step(dev):
    """IMU_Net's forward in the split3 mode, then one timed U+L training step (ConcurrentStages, HIP graph) -> its outputs on the CPU."""
    import bench
    from mmego_amd import nets
    from mmego_amd.train_step import ConcurrentStages, StageStep
    with torch.cuda.device(dev):
        imu = torch.randn(16, 8, 20, 15, generator=torch.Generator().manual_seed(2)).to(dev)
        torch.manual_seed(41)
        net = nets.IMUNet(15, 9, 512, 2, True, 0.1).to(dev).eval()
        net.precision = "split3"
        with torch.no_grad():
            out = list(net(imu))
        x, imu_in, body, target = [v.to(dev) for v in bench.synth_batch(1234, "cpu")]
        himu, hup, hlo, hfr = bench.build_hip_models(dev)
        himu_l = bench.clone_imu(himu, dev)
        bench._lstm_dropout_off(hup, hlo)
        su = StageStep("upper", hup, himu, lr=3e-5, use_graph=True)
        sl = StageStep("lower", hlo, himu_l, upper_frozen=hfr, lr=3e-5, use_graph=True)
        su.bind(x, imu_in, body, target)
        sl.bind(x, imu_in, body, target)
        ConcurrentStages([su, sl], use_graph=True).step()
        torch.cuda.synchronize()
        out += [t for st in (su, sl) for t in (st.net.flat().flat_g, st.net.flat().flat_p)]
        return [t.detach().cpu() for t in out]


def test_split3_forward_and_ul_step_are_bit_identical_on_two_devices():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices (%d visible)" % torch.cuda.device_count())
    from mmego_amd import blocks, hip
    hip.lib()
    first = _split3_forward_and_ul_step(torch.device("cuda:0"))
    second = _split3_forward_and_ul_step(torch.device("cuda:1"))
    names = ["R", "t", "upper grad", "upper params", "lower grad", "lower params"]
    for name, a, b in zip(names, first, second):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert blocks.seq_xcd_errors() == 0
