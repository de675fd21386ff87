"""GPU: --finetune_imu -- IMU_Net trained end to end through Upper_Net's head-pose gradients (Train_Upper.py:162 without its .detach()).

One step of train_step.StageStep("upper", finetune_imu=True) against the CPU oracle's autograd through both nets, eager against graph
replay, and the command line on the synthetic data tree of tests/test_cli_gpu.py."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, set_lstm_dropout

pytestmark = pytest.mark.gpu

NOISE_GRAD = re.compile(r"(conv[123]\.bias|tcn\.2\.bias|residual\.0\.bias|attn\.bias|to_k\.bias|fusion\.attn\.weight)$")
LR, IMU_LR = 3e-5, 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _hip_stage(dev, sd_imu, sd_up, batch, use_graph):
    from mmego_amd import nets
    from mmego_amd.train_step import StageStep
    himu = nets.IMUNet(15, 9, 512, 2, True, 0)
    himu.load_state_dict(sd_imu)
    himu = himu.to(dev).train()
    hup = nets.UpperNet()
    hup.load_state_dict(sd_up)
    hup = hup.to(dev).train()
    hup.lstm_dropout = 0
    st = StageStep("upper", hup, himu, lr=LR, use_graph=use_graph, finetune_imu=True, imu_lr=IMU_LR)
    x, imu, body, target = [v.to(dev) for v in batch]
    st.bind(x, imu, body, target)
    return st


def test_finetune_step_against_oracle(dev):
    """B=4, T=8, N=128, IMU_Net(15, 9, 512, 2, True, 0) -> Upper_Net without detach on both sides (oracle: fp32, CPU, one thread).
    Every IMU_Net gradient within 2e-4 of the largest IMU_Net gradient (the bar of test_imu_stage1_gradients_at_full_size), every
    Upper_Net gradient within 2e-4 of the largest Upper_Net gradient (_compare_training); after the two Adam steps (Upper_Net at lr,
    IMU_Net at imu_lr with weight decay 1e-3) the parameters as test_ul_step_at_bench_shape_against_oracle compares them: at most one
    +-lr flip of a ~0 gradient's sign, fewer than 5 % of the elements moved at all, fc3 (Q7) untouched; graph replay == eager, bit
    for bit, over two steps."""
    from mmego_amd import blocks
    from mmego_amd.train_step import ConcurrentStages, StageStep
    from oracle import nets as on
    from oracle import skeleton as sk
    from oracle import train as ot
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        B, T, N = 4, 8, 128
        torch.manual_seed(41)
        oimu = on.IMUNet(15, 9, 512, 2, True, 0).train()
        oup = on.UpperNet().train()
        set_lstm_dropout(oup, 0.0)
        sd_imu = {k: v.clone() for k, v in oimu.state_dict().items()}
        sd_up = {k: v.clone() for k, v in oup.state_dict().items()}
        g = torch.Generator().manual_seed(42)
        x = torch.randn(B, T, N, 6, generator=g)
        imu = torch.randn(B, T, 20, 15, generator=g)
        body = torch.randn(B, 20, 3, generator=g) * 0.3
        target = torch.randn(B, T, 21, 3, generator=g)
        batch = (x, imu, body, target)

        h0, c0 = ot.zeros_state(B)
        R, t = oimu(imu)                                             # (no torch.no_grad(), no .detach(): the fine-tuning body)
        lo = oup(x.clone(), h0, c0, body, R, t)[0]
        loss_o = ot.l1_sum(lo, target[:, :, list(sk.UPPER_MAP)])
        loss_o.backward()

        st = _hip_stage(dev, sd_imu, sd_up, batch, use_graph=False)
        st.step()
        torch.cuda.synchronize()
        assert abs(st.loss.item() - loss_o.item()) < 2e-5 * abs(loss_o.item()), (st.loss.item(), loss_o.item())
        assert torch.allclose(st.last_pred.cpu(), lo.detach(), rtol=1e-4, atol=2e-5)
        for tag, o, h in (("imu", oimu, st.imu), ("upper", oup, st.net)):
            po, ph = dict(o.named_parameters()), dict(h.named_parameters())
            flat = h.flat()
            scale = max(p.grad.abs().max().item() for p in po.values() if p.grad is not None)
            worst = 0.0
            for k in po:
                go = po[k].grad if po[k].grad is not None else torch.zeros_like(po[k])
                err = (flat.grad(ph[k]).detach().cpu() - go).abs().max().item()
                worst = max(worst, err)
                assert err < 2e-4 * scale, (tag, k, err, scale)
            print("finetune step: %s gradients, worst error %.3e at scale %.3e (%.2e of it)" % (tag, worst, scale, worst / scale))
        assert oimu.fc3.weight.grad is None

        # the two Adam steps
        torch.optim.Adam(oup.parameters(), lr=LR).step()
        torch.optim.Adam(oimu.parameters(), lr=IMU_LR, weight_decay=0.001).step()
        for tag, o, h, lr in (("imu", oimu, st.imu, IMU_LR), ("upper", oup, st.net, LR)):
            n_bad = n_all = 0
            sd_o, sd_h = o.state_dict(), h.state_dict()
            for k, p in o.named_parameters():
                if NOISE_GRAD.search(k):
                    continue
                dp = (sd_h[k].cpu() - sd_o[k]).abs()
                assert dp.max().item() <= 2 * lr + 2e-6, (tag, k, dp.max().item())
                n_bad += int((dp > 2e-6).sum())
                n_all += dp.numel()
            print("finetune step: %s parameters, %d of %d moved by more than 2e-6" % (tag, n_bad, n_all))
            assert n_bad < 0.05 * n_all, (tag, n_bad, n_all)
        for k in ("fc3.weight", "fc3.bias"):
            assert torch.equal(st.imu.state_dict()[k].cpu(), sd_imu[k]), k
        moved = [k for k, v in st.imu.state_dict().items() if not torch.equal(v.cpu(), sd_imu[k])]
        assert len(moved) == len(sd_imu) - 2, "every IMU_Net tensor but fc3 is trained"

        # graph replay == eager, bit for bit (two steps: the second replays the captured graph on updated weights)
        res = []
        for use_graph in (False, True):
            s2 = _hip_stage(dev, sd_imu, sd_up, batch, use_graph=use_graph)
            losses = []
            for _ in range(2):
                losses.append(s2.step().item())
            torch.cuda.synchronize()
            assert (s2.graph is not None) == use_graph
            res.append((losses, s2.net.flat().flat_g.clone(), s2.net.flat().flat_p.clone(), s2.imu.flat().flat_g.clone(),
                        s2.imu.flat().flat_p.clone(), [b.clone() for b in s2.net.buffers()]))
        assert res[0][0] == res[1][0], (res[0][0], res[1][0])
        for a, b in zip(res[0][1:5], res[1][1:5]):
            assert torch.equal(a, b)
        for a, b in zip(res[0][5], res[1][5]):
            assert torch.equal(a, b)
        assert blocks.seq_xcd_errors() == 0

        # the engines built around a frozen, shareable IMU_Net forward refuse such a stage
        with pytest.raises(ValueError, match="finetune_imu"):
            ConcurrentStages([s2])
        with pytest.raises(ValueError, match="finetune_imu"):
            StageStep("lower", s2.net, s2.imu, finetune_imu=True)
    finally:
        torch.set_num_threads(threads)


def test_cli_finetune_one_epoch(tmp_path):
    """main.py --train --network Upper_Net --finetune_imu --epochs 1 --seed 0 from a saved random IMU_Net checkpoint: both
    checkpoints written and loadable, the IMU_Net's weights moved, fc3 untouched (never trained, Q7), the logged losses finite; the same
    command without the flag writes no IMU_Net and leaves the checkpoint it loaded alone."""
    from test_cli_gpu import _make_dataset, _run
    from mmego_amd import nets
    data = str(tmp_path / "Sample_data")
    _make_dataset(data, np.random.default_rng(3))
    torch.manual_seed(2)
    imu_ck = str(tmp_path / "imu.pth")
    start = nets.IMUNet(15, 9, 512, 2, True, 0.1).state_dict()
    torch.save(start, imu_ck)
    start = {k: v.clone() for k, v in start.items()}
    out_dir = str(tmp_path / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    common = ["--train", "--network", "Upper_Net", "--load_IMU_path", imu_ck, "--data_root", data, "--epochs", "1", "--batch_size", "3",
              "--device", "cuda:0", "--seed", "0"]
    out = _run(common + ["--finetune_imu", "--imu_lr", "1e-4", "--log_dir", "9141"], env)
    assert "epoch: 1" in out and "Average Joint Localization Error" in out
    mdir = os.path.join(out_dir, "model", "9141")
    up = [f for f in glob.glob(os.path.join(mdir, "epoch0_batch3frame*.pth")) if not f.endswith(".train_state.pth")]
    im = glob.glob(os.path.join(mdir, "IMU_Net", "epoch0_batch3frame*.pth"))
    assert len(up) == 1 and len(im) == 1, (os.listdir(mdir))
    assert os.path.basename(up[0]) == os.path.basename(im[0])
    nets.UpperNet().load_state_dict(torch.load(up[0], map_location="cpu"))
    got = torch.load(im[0], map_location="cpu")
    nets.IMUNet(15, 9, 512, 2, True, 0).load_state_dict(got)
    assert got.keys() == start.keys()
    for k in start:
        assert bool(torch.isfinite(got[k]).all()), k
        if k.startswith("fc3."):
            assert torch.equal(got[k], start[k]), k
        else:
            assert not torch.equal(got[k], start[k]), k
    log = open(os.path.join(out_dir, "report", "9141", "log-loss.txt")).read().split()
    assert np.isfinite(float(log[1]))
    # without the flag: the IMU_Net is frozen -- nothing saved for it, the loaded checkpoint as it was
    out = _run(common + ["--log_dir", "9142"], env)
    assert "epoch: 1" in out
    assert not os.path.exists(os.path.join(out_dir, "model", "9142", "IMU_Net"))
    after = torch.load(imu_ck, map_location="cpu")
    for k in start:
        assert torch.equal(after[k], start[k]), k


def test_finetune_step_honours_train_precision_split3(dev):
    """IMUNet.train_precision = "split3" under fine-tuning (B=64, T=8: the row counts where imu_train takes the piece products): the
    body really runs bf16-MFMA entry points, none of its launches is unordered against one of them (the structural check of
    tests/test_split3_gpu.py on the recorded launch / wait graph), and both nets' gradients stay within 2e-4 of their largest entry
    of the fp32 body's."""
    from mmego_amd import hip
    from mmego_amd.plan import StepPlan
    B, T, N = 64, 8, 128
    torch.manual_seed(51)
    from mmego_amd import nets
    sd_imu = {k: v.clone() for k, v in nets.IMUNet(15, 9, 512, 2, True, 0).state_dict().items()}
    sd_up = {k: v.clone() for k, v in nets.UpperNet().state_dict().items()}
    g = torch.Generator().manual_seed(52)
    batch = (torch.randn(B, T, N, 6, generator=g), torch.randn(B, T, 20, 15, generator=g), torch.randn(B, 20, 3, generator=g) * 0.3,
             torch.randn(B, T, 21, 3, generator=g))
    grads = {}
    for prec in ("fp32", "split3"):
        st = _hip_stage(dev, sd_imu, sd_up, batch, use_graph=False)
        st.imu.train_precision = prec
        st._body()
        torch.cuda.synchronize()
        grads[prec] = (st.imu.flat().flat_g.clone(), st.net.flat().flat_g.clone())
        if prec == "split3":
            plan = StepPlan().record(st._body)
            assert sum(hip.is_bf16_mfma_entry(n) for sg in plan.segments for n, _ in sg.calls) >= 8
            assert plan.unordered_with(hip.is_bf16_mfma_entry) == []
    for i, tag in enumerate(("imu", "upper")):
        a, b = grads["fp32"][i], grads["split3"][i]
        scale = float(a.abs().max())
        err = float((a - b).abs().max())
        print("finetune split3 vs fp32: %s gradients %.3e at scale %.3e" % (tag, err, scale))
        assert err < 2e-4 * scale, (tag, err, scale)
    assert not torch.equal(grads["fp32"][0], grads["split3"][0])          # (the modes are really different arithmetic)
