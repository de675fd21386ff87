"""GPU: train_step.ImuStep(imu_noise=...) and StageStep(imu_noise=...) -- the IMU samples perturbed inside the (captured) step body by
mmego_imu_jitter -- against a noise-free step that is FED the samples ops.imu_jitter makes at the same key: losses, gradients, the
parameters and the Adam state bit for bit.  B=2, T=3, nets from torch.manual_seed, IMU_Nets of hidden size 64, N=32 points."""
import pytest
import torch

import step_helpers
from step_helpers import raw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, T, N = 2, 3, 32
SIGMAS = (1.0, 0.05, 0.01, 2.0, 0.2, 0.02)
KEYS = (0x1234567890ABCDEF, 6, 2 ** 63 + 7)                                        # (the last: only its low 63 bits count)


def _batch(seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, N, 6, generator=g)
    x[:, ::2, N - N // 4:] = 0.0                                                  # (the loader's zero padding)
    imu = torch.randn(B, T, 20, 15, generator=g)
    imu[..., :9] = torch.linalg.qr(torch.randn(B, T, 20, 3, 3, generator=g))[0].reshape(B, T, 20, 9)
    body = torch.randn(B, 20, 3, generator=g) * 0.3
    target = torch.randn(B, T, 21, 3, generator=g)
    R = torch.linalg.qr(torch.randn(B, T, 3, 3, generator=g))[0].contiguous()
    return [v.to(DEV) for v in (x, imu, body, target, R)]


def _build(kind, use_graph=True, seed=1000, **kw):
    """kind "imu": the stage-1 step (LSTM dropout 0.1); "finetune": the Upper stage training its IMU_Net; "frozen": the Upper stage with a
    frozen IMU_Net of its own -> (step bound to a fresh batch, its nets, the bound IMU samples)."""
    from mmego_amd import nets
    from mmego_amd.train_step import ImuStep, StageStep
    torch.manual_seed(seed)
    x, imu, body, target, R = _batch()
    if kind == "imu":
        net = nets.IMUNet(15, 9, 64, 2, True, 0.1).to(DEV).train()
        st = ImuStep(net, lr=1e-4, use_graph=use_graph, **kw)
        st.bind(imu, R, target)
        return st, [net], imu
    up = nets.UpperNet().to(DEV).train()
    if kind == "finetune":
        imu_net = nets.IMUNet(15, 9, 64, 2, True, 0).to(DEV).train()
        st = StageStep("upper", up, imu_net, lr=3e-5, use_graph=use_graph, finetune_imu=True, imu_lr=1e-5, **kw)
    else:
        imu_net = nets.IMUNet(15, 9, 64, 2).to(DEV).eval()
        st = StageStep("upper", up, imu_net, lr=3e-5, use_graph=use_graph, **kw)
    st.bind(x, imu, body, target)
    return st, [up, imu_net], imu


def _left_behind(st, nets_):
    return [(k, raw(v).clone()) for k, v in step_helpers.state(st, nets_)]


def _same(a, b):
    assert [k for k, _ in a] == [k for k, _ in b]
    for (k, x), (_, y) in zip(a, b):
        assert torch.equal(x, y), k


def _by_hand(imu, key):
    """The samples perturbed by ops.imu_jitter at ``key``: what the noisy step makes inside its body."""
    from mmego_amd import ops
    word = torch.tensor([key & 0x7FFFFFFFFFFFFFFF], dtype=torch.int64, device=DEV)
    return ops.imu_jitter(imu, SIGMAS, word, torch.empty_like(imu))


def _noisy_against_fed(kind, use_graph=True):
    """One step, and again three steps under three keys, from the same state."""
    for keys in (KEYS[:1], KEYS):
        st, nets_, imu = _build(kind, use_graph, imu_noise=SIGMAS)
        clean = imu.clone()
        ref, ref_nets, ref_in = _build(kind, use_graph)
        for (_, a, _), (_, b, _) in zip(step_helpers.trained(st), step_helpers.trained(ref)):
            assert torch.equal(a.flat().flat_p, b.flat().flat_p)                  # both start from the same state
        for k in keys:
            st.set_imu_key(k)
            st.step()
            ref_in.copy_(_by_hand(clean, k))
            ref.step()
        torch.cuda.synchronize()
        got = _left_behind(st, nets_)
        _same(got, _left_behind(ref, ref_nets))
        assert torch.equal(imu, clean), "the bound input buffer is never written"
        assert int(st.imu_word.item()) == keys[-1] & 0x7FFFFFFFFFFFFFFF
        assert torch.equal(st._imu_out[tuple(imu.shape)], _by_hand(clean, keys[-1]))
    # and the noise did something: the clean samples give other bits
    plain, plain_nets, _ = _build(kind, use_graph)
    for _ in KEYS:
        plain.step()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b) for (_, a), (_, b) in zip(got, _left_behind(plain, plain_nets)))


@pytest.mark.parametrize("use_graph", [True, False])
def test_imu_step_equals_the_fed_samples(use_graph):
    _noisy_against_fed("imu", use_graph)


def test_finetune_imu_stage_equals_the_fed_samples():
    _noisy_against_fed("finetune")


def test_frozen_imu_stage_equals_the_fed_samples():
    _noisy_against_fed("frozen")


@pytest.mark.parametrize("kind", ["imu", "frozen"])
def test_keys_draw_afresh_and_reproduce(kind):
    """Graph replay with a rewritten key changes the result; the same keys from a restored state reproduce it."""
    def run(keys):
        st, nets_, _ = _build(kind, True, imu_noise=SIGMAS)
        out = []
        for k in keys:
            st.set_imu_key(k)
            st.step()
            torch.cuda.synchronize()
            out.append((getattr(st, "loss2", st.loss).cpu().clone(), _left_behind(st, nets_)))
        assert st.graph is not None
        return out
    a, b, c = run((5, 6)), run((5, 6)), run((5, 5))
    for (la, sa), (lb, sb) in zip(a, b):
        assert torch.equal(la, lb)
        _same(sa, sb)
    assert torch.equal(a[0][0], c[0][0]) and not torch.equal(a[1][0], c[1][0]), "the second step's key is what differs"


def test_option_off_launches_what_it_launched():
    """imu_noise=None: no extra buffer, no word, and the body's entry points are the noisy body's less its one mmego_imu_jitter."""
    for kind in ("imu", "finetune", "frozen"):
        st, _, imu = _build(kind, False)
        st.step()
        torch.cuda.synchronize()
        off = step_helpers.entry_points(st._body)
        assert len(off) > 20 and "imu_jitter" not in off
        assert st.imu_noise is None and not hasattr(st, "imu_word") and not hasattr(st, "_imu_out")
        if kind == "imu":
            assert set(st.static) == {"imu", "R_gt", "target", "head", "dR", "dt"}
        else:
            assert set(st.static) == {"x_src", "x", "imu", "body", "target", "h0", "c0", "dl", "R_gt", "t_gt"}
        on, _, imu = _build(kind, False, imu_noise=SIGMAS)
        on.set_imu_key(1)
        on.step()
        torch.cuda.synchronize()
        with_noise = step_helpers.entry_points(on._body)
        assert with_noise.count("imu_jitter") == 1
        assert [n for n in with_noise if n != "imu_jitter"] == off, kind
        assert set(on.static) == set(st.static)
        assert on.imu_word.dtype == torch.int64 and tuple(on.imu_word.shape) == (1,) and on.imu_word.is_cuda
        assert list(on._imu_out) == [tuple(imu.shape)]
        on.bind(*([imu, on.static["R_gt"], on.static["target"]] if kind == "imu" else
                  [on.static["x_src"], imu, on.static["body"], on.static["target"]]))
        assert list(on._imu_out) == [tuple(imu.shape)], "one output buffer per bound minibatch shape"


def test_a_stage_without_an_imu_net_of_its_own_refuses():
    from mmego_amd import nets
    from mmego_amd.train_step import ImuStep, PipelinedStages, SharedImuStages, StageStep
    torch.manual_seed(3)
    x, imu, body, target, R = _batch()
    up, lo = nets.UpperNet().to(DEV).train(), nets.LowerNet(64).to(DEV).train()
    imu_net = nets.IMUNet(15, 9, 64, 2).to(DEV).eval()
    pose = (torch.empty(B, T, 3, 3, device=DEV), torch.empty(B, T, 3, device=DEV))
    with pytest.raises(ValueError, match="imu_noise"):
        StageStep("upper", up, None, imu_noise=SIGMAS)                             # the recorded pose
    with pytest.raises(ValueError, match="imu_noise"):
        StageStep("upper", up, imu_net, pose=pose, imu_noise=SIGMAS)               # a shared pose
    with pytest.raises(ValueError, match="imu_noise"):
        StageStep("lower", lo, None, upper_frozen=up, imu_noise=SIGMAS)
    for bad in ((0.0,) * 6, (1.0,) * 5, (-1.0, 0, 0, 0, 0, 0), (float("nan"), 1, 1, 1, 1, 1), (float("inf"), 0, 0, 0, 0, 0)):
        with pytest.raises(ValueError, match="imu_noise"):
            StageStep("upper", up, imu_net, imu_noise=bad)
        with pytest.raises(ValueError, match="imu_noise"):
            ImuStep(nets.IMUNet(15, 9, 64, 2, True, 0).to(DEV).train(), imu_noise=bad)
    # the engines that give a stage somebody else's pose refuse a stage under the option
    st = StageStep("upper", up, imu_net, use_graph=False, imu_noise=SIGMAS)
    with pytest.raises(ValueError, match="imu_noise"):
        SharedImuStages(imu_net, [st], imu)
    with pytest.raises(ValueError):
        PipelinedStages([st], [nets.IMUNet(15, 9, 64, 2).to(DEV).eval()], imu)
    assert st.pose is None
    # and composes with the head-pose noise where the IMU_Net is frozen
    both = StageStep("upper", up, imu_net, use_graph=False, imu_noise=SIGMAS, pose_noise_deg=1.0)
    assert both.imu_noise == SIGMAS and both.pose_noise == (1.0, 0.0)
