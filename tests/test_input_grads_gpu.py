"""GPU: the head-pose gradients of Upper_Net (d loss / d R, d loss / d t) against the float64 CPU oracle, the kernels behind them
against float64 formulas, and what must NOT change for callers whose pose is detached.

Bar for gradients: the one tests/test_hip_parity.py::_compare_training holds first-step gradients to -- max abs error below 2e-4 of
the largest entry of that gradient.  The fp32 oracle itself sits within 4e-6 of the float64 oracle on that scale at these shapes, so the
bar leaves fp32 rounding a factor of ~50: a miss is a bug.
"""
import json
import os

import pytest
import torch

from conftest import GOLDEN, set_lstm_dropout
from oracle import geometry as geo
from oracle import nets as on
from oracle import skeleton as sk
from oracle import train as ot
from step_helpers import entry_points as _entry_points

pytestmark = pytest.mark.gpu

GRAD_BAR = 2e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _pair(dev, seed):
    """The oracle in float64 and the HIP net with the same weights, train mode, LSTM dropout off on both sides."""
    from mmego_amd import nets
    torch.manual_seed(seed)
    o = on.UpperNet().train()
    h = nets.UpperNet().to(dev).train()
    h.load_state_dict({k: v.to(dev) for k, v in o.state_dict().items()})
    set_lstm_dropout(o, 0.0)
    set_lstm_dropout(h, 0.0)
    h.lstm_dropout = 0
    return o.double(), h


def _batch(seed, B, T, N, orthonormal, padded):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, N, 6, generator=g)
    if padded:                       # the loader's zero padding: whole rows of zeros behind a frame's real points
        x[:, ::2, N // 2:] = 0.0
        x[1, :, N // 4:] = 0.0
    body = torch.randn(B, 20, 3, generator=g) * 0.3
    R = geo.rot6d_imu(torch.randn(B * T, 6, generator=g)).view(B, T, 3, 3).contiguous()
    if not orthonormal:
        R = R + 1e-2 * torch.randn(B, T, 3, 3, generator=g)
    t = torch.randn(B, T, 3, generator=g)
    target = torch.randn(B, T, 15, 3, generator=g)
    return x, body, R, t, target


def _oracle_grads(o, x, body, R, t, target):
    """float64 CPU oracle with both pose tensors requiring grad -> (joints, dR, dt, {name: parameter gradient})."""
    B = x.shape[0]
    Rd, td = R.double().requires_grad_(), t.double().requires_grad_()
    h0, c0 = [v.double() for v in ot.zeros_state(B)]
    for p in o.parameters():
        p.grad = None
    l = o(x.double().clone(), h0, c0, body.double(), Rd, td)[0]
    ot.l1_sum(l, target.double()).backward()
    return l.detach(), Rd.grad, td.grad, {k: p.grad for k, p in o.named_parameters()}


def _hip_grads(h, dev, x, body, R, t, target, need_R=True, need_t=True):
    B = x.shape[0]
    Rh, th = R.to(dev).requires_grad_(need_R), t.to(dev).requires_grad_(need_t)
    h0, c0 = [v.to(dev) for v in ot.zeros_state(B)]
    for p in h.parameters():
        p.grad = None
    l = h(x.to(dev).clone(), h0, c0, body.to(dev), Rh, th)[0]
    (l - target.to(dev)).abs().sum().backward()
    torch.cuda.synchronize()
    return l.detach(), Rh.grad, th.grad, {k: p.grad.clone() for k, p in h.named_parameters()}


def _rel_err(got, want):
    return float((got.double().cpu() - want).abs().max()), float(want.abs().max())


def test_upper_head_pose_gradients_against_oracle(dev):
    """B=4, T=8, train mode, loss L1(sum) on the 15 joints.  Cases: orthonormal R and R perturbed by 1e-2 noise (NOT orthonormal: the
    head-frame share must come from the untransformed points, never from R^T p'); only R / only t / both requiring grad; N = 64 and
    256 once each; a batch with zero-padded points (transformed like any other point: p' = -R t, and they contribute)."""
    B, T = 4, 8
    cases = [  # (N, orthonormal, need_R, need_t, padded)
        (128, True, True, True, False),
        (128, False, True, True, False),
        (128, True, True, False, False),
        (128, True, False, True, False),
        (64, False, True, True, False),
        (256, True, True, True, False),
        (128, False, True, True, True),
    ]
    o, h = _pair(dev, 11)
    before = {k: v.clone() for k, v in o.state_dict().items()}
    for i, (N, orth, need_R, need_t, padded) in enumerate(cases):
        o.load_state_dict(before)                                          # (BatchNorm running statistics: every case from the same state)
        h.load_state_dict({k: v.float().to(dev) for k, v in before.items()})
        x, body, R, t, target = _batch(100 + i, B, T, N, orth, padded)
        lo, dRo, dto, _ = _oracle_grads(o, x, body, R, t, target)
        lh, dRh, dth, _ = _hip_grads(h, dev, x, body, R, t, target, need_R, need_t)
        tag = (N, orth, need_R, need_t, padded)
        print("case", tag, "joints max err %.3e" % float((lh.double().cpu() - lo).abs().max()))
        assert torch.allclose(lh.cpu(), lo.float(), rtol=1e-4, atol=2e-5), (tag, float((lh.double().cpu() - lo).abs().max()))
        assert (dRh is not None) == need_R and (dth is not None) == need_t, tag
        if need_R:
            assert dRh.shape == R.shape and dRh.dtype == torch.float32
            err, scale = _rel_err(dRh, dRo)
            print("   dR max err %.3e at scale %.3e (%.2e of it)" % (err, scale, err / scale))
            assert err < GRAD_BAR * scale, (tag, "dR", err, scale)
        if need_t:
            assert dth.shape == t.shape and dth.dtype == torch.float32
            err, scale = _rel_err(dth, dto)
            print("   dt max err %.3e at scale %.3e (%.2e of it)" % (err, scale, err / scale))
            assert err < GRAD_BAR * scale, (tag, "dt", err, scale)


def test_head_pose_gradients_are_reproducible_and_free_when_unused(dev):
    """Two runs give dR, dt bit for bit (fixed-order reductions, no atomics); asking for the pose gradients does not change a bit of
    the parameter gradients; and a training step whose pose is detached launches exactly what it launched before this feature
    (tests/golden/upper_step_entry_points.json: the recorded entry points of StageStep("upper")._body, B=4, T=8, N=128, recorded head
    pose, written down on the commit before the pose gradients existed)."""
    from mmego_amd import nets
    from mmego_amd.train_step import StageStep
    B, T, N = 4, 8, 128
    _, h = _pair(dev, 12)
    state = {k: v.clone() for k, v in h.state_dict().items()}
    x, body, R, t, target = _batch(200, B, T, N, False, True)
    runs = []
    for need in (True, True, False):
        h.load_state_dict(state)
        runs.append(_hip_grads(h, dev, x, body, R, t, target, need, need))
    (l0, dR0, dt0, p0), (l1, dR1, dt1, p1), (l2, dR2, dt2, p2) = runs
    assert torch.equal(dR0, dR1) and torch.equal(dt0, dt1) and torch.equal(l0, l1)
    assert dR2 is None and dt2 is None and torch.equal(l0, l2)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
        assert torch.equal(p0[k], p2[k]), k                      # with / without requires_grad on the pose
    assert float(dR0.abs().max()) > 0 and float(dt0.abs().max()) > 0

    # the default step's launch sequence
    torch.manual_seed(3)
    net = nets.UpperNet().to(dev).train()
    g = torch.Generator().manual_seed(4)
    xs = torch.randn(B, T, N, 6, generator=g).to(dev)
    tgt = torch.randn(B, T, 21, 3, generator=g).to(dev)
    st = StageStep("upper", net, None, use_graph=False)
    st.bind(xs, None, body.to(dev), tgt, R_gt=R.to(dev))
    st.step()
    torch.cuda.synchronize()
    names = _entry_points(st._body)
    want = json.load(open(os.path.join(GOLDEN, "upper_step_entry_points.json")))
    assert names == want["entry_points"], [(i, a, b) for i, (a, b) in enumerate(zip(names, want["entry_points"])) if a != b][:5]
    assert getattr(net, "_pose", None) is None                   # no extra buffer kept
    assert not any(net.arena("train").has(k) for k in ("pts_raw", "dR", "dt", "m0.dy0"))


def _f64(v):
    return v.double().cpu()


def test_new_kernels_against_float64(dev):
    """mmego_transform2h_backward and the world-transform pose gradients (mmego_head_fk_backward_pose, mmego_head_fk_loss_pose) alone,
    against the formulas in float64 on random data; the existing outputs of the two head_fk variants bit-equal to the entry points
    they extend."""
    from mmego_amd import hip
    g = torch.Generator().manual_seed(21)
    for F in (1, 33, 512):
        for N in (64, 128, 256):
            pts = torch.randn(F * N, 6, generator=g).to(dev)
            pts[N // 2:N] = 0.0                                                     # (zero-padded rows contribute like any other)
            R = (geo.rot6d_imu(torch.randn(F, 6, generator=g)) + 1e-2 * torch.randn(F, 3, 3, generator=g)).contiguous().to(dev)
            t = torch.randn(F, 3, generator=g).to(dev)
            ga = torch.randn(F * N, 28, generator=g).to(dev)                        # row-strided sources, as in the net
            gb = torch.randn(F * N, 6, generator=g).to(dev)
            d = (_f64(pts)[:, :3].view(F, N, 3) - _f64(t)[:, None, :])
            for two in (False, True):
                gsum = (_f64(ga)[:, :3] + (_f64(gb)[:, :3] if two else 0)).view(F, N, 3)
                want_R = torch.einsum("fni,fnk->fik", gsum, d)
                want_t = -torch.einsum("fik,fi->fk", _f64(R), gsum.sum(1))
                dR = torch.full((F, 3, 3), 7.0, device=dev)
                dt = torch.full((F, 3), 7.0, device=dev)
                hip.call("transform2h_backward", pts, 6, F, N, R, t, ga, 28, gb if two else None, 6, 0, dR, dt)
                for name, got, want in (("dR", dR, want_R), ("dt", dt, want_t)):
                    err, scale = _rel_err(got, want)
                    print("transform2h_backward F=%d N=%d two=%d %s: %.3e at scale %.3e" % (F, N, two, name, err, scale))
                    assert err < GRAD_BAR * scale, (F, N, two, name, err, scale)
                # accumulate: added to what the buffers hold; and a second run gives the same bits
                base_R, base_t = torch.randn(F, 3, 3, generator=g).to(dev), torch.randn(F, 3, generator=g).to(dev)
                acc_R, acc_t = base_R.clone(), base_t.clone()
                hip.call("transform2h_backward", pts, 6, F, N, R, t, ga, 28, gb if two else None, 6, 1, acc_R, acc_t)
                assert torch.equal(acc_R, base_R + dR) and torch.equal(acc_t, base_t + dt)
                dR2, dt2 = torch.empty_like(dR), torch.empty_like(dt)
                hip.call("transform2h_backward", pts, 6, F, N, R, t, ga, 28, gb if two else None, 6, 0, dR2, dt2)
                assert torch.equal(dR2, dR) and torch.equal(dt2, dt)
        # world transform: world = Rw^T joint + tw  ->  dtw = sum_slots dj, dRw[k][i] = sum_slots joint_k dj_i
        B = 4 if F % 4 == 0 else 1
        y = torch.randn(F, 87, generator=g).to(dev)
        body = (torch.randn(B, 20, 3, generator=g) * 0.3).to(dev)
        Rw = (geo.rot6d_imu(torch.randn(F, 6, generator=g)) + 1e-2 * torch.randn(F, 3, 3, generator=g)).contiguous().to(dev)
        tw = torch.randn(F, 3, generator=g).to(dev)
        q, jh, world = torch.empty(F, 14, 3, 3, device=dev), torch.empty(F, 15, 3, device=dev), torch.empty(F, 15, 3, device=dev)
        hip.call("head_fk_forward", 0, y, body, B, F, q, jh, Rw, tw, world, None, 0, None)
        dj = torch.randn(F, 15, 3, generator=g).to(dev)
        dy0, dy1 = torch.empty(F, 87, device=dev), torch.empty(F, 87, device=dev)
        dRw, dtw = torch.empty(F, 3, 3, device=dev), torch.empty(F, 3, device=dev)
        hip.call("head_fk_backward", 0, y, body, B, F, dj, dy0, Rw)
        hip.call("head_fk_backward_pose", 0, y, body, B, F, dj, dy1, Rw, jh, dRw, dtw)
        assert torch.equal(dy0, dy1)
        want_R = torch.einsum("fsk,fsi->fki", _f64(jh), _f64(dj))
        want_t = _f64(dj).sum(1)
        for name, got, want in (("dRw", dRw, want_R), ("dtw", dtw, want_t)):
            err, scale = _rel_err(got, want)
            print("head_fk_backward_pose F=%d %s: %.3e at scale %.3e" % (F, name, err, scale))
            assert err < GRAD_BAR * scale, (F, name, err, scale)
        # the fused loss launch: same bits as without the pose outputs, and the pose gradients of ITS loss gradient (the sign)
        target = torch.randn(F, 21, 3, generator=g).to(dev)
        jmap = torch.tensor(sk.UPPER_MAP, dtype=torch.int32, device=dev)
        nb = (F + 63) // 64
        outs = []
        for pose in (False, True):
            scr = torch.zeros(2 * nb + 1, dtype=torch.float64, device=dev)
            q2, jh2, w2 = torch.empty_like(q), torch.empty_like(jh), torch.empty_like(world)
            loss2, dy2 = torch.zeros(2, device=dev), torch.empty(F, 87, device=dev)
            pR, pt = torch.empty(F, 3, 3, device=dev), torch.empty(F, 3, device=dev)
            if pose:
                hip.call("head_fk_loss_pose", 0, y, body, B, F, q2, jh2, Rw, tw, w2, None, 0, None, target, jmap, 21, 1.0, loss2, dy2, scr, pR, pt)
            else:
                hip.call("head_fk_loss", 0, y, body, B, F, q2, jh2, Rw, tw, w2, None, 0, None, target, jmap, 21, 1.0, loss2, dy2, scr)
            outs.append((q2, jh2, w2, loss2, dy2, pR, pt))
        for a, b in zip(outs[0][:5], outs[1][:5]):
            assert torch.equal(a, b)
        assert torch.equal(outs[0][2], world)
        sign = torch.sign(_f64(world) - _f64(target)[:, list(sk.UPPER_MAP)])
        want_R = torch.einsum("fsk,fsi->fki", _f64(jh), sign)
        want_t = sign.sum(1)
        for name, got, want in (("dRw", outs[1][5], want_R), ("dtw", outs[1][6], want_t)):
            err, scale = _rel_err(got, want)
            print("head_fk_loss_pose F=%d %s: %.3e at scale %.3e" % (F, name, err, scale))
            assert err < GRAD_BAR * scale, (F, name, err, scale)


def test_lower_and_wlocal_refuse_differentiable_pose(dev):
    """Lower_Net and UpperNetwlocal produce no input gradients: a pose (or, for Lower_Net, an upper_l) that requires grad raises
    instead of silently losing its gradient; with grad disabled, or detached, the call goes through."""
    from mmego_amd import nets, nets_local
    B, T, N = 2, 4, 128
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, T, N, 6, generator=g).to(dev)
    body = (torch.randn(B, 20, 3, generator=g) * 0.3).to(dev)
    R = geo.rot6d_imu(torch.randn(B * T, 6, generator=g)).view(B, T, 3, 3).contiguous().to(dev)
    t = torch.randn(B, T, 3, generator=g).to(dev)
    up = torch.randn(B, T, 15, 3, generator=g).to(dev)
    h0, c0 = [v.to(dev) for v in ot.zeros_state(B)]
    torch.manual_seed(5)
    low = nets.LowerNet(64).to(dev).train()
    wl = nets_local.UpperNetwlocal().to(dev).train()
    for name in ("R", "t", "upper_l"):
        a = dict(R=R.clone(), t=t.clone(), upper_l=up.clone())
        a[name].requires_grad_()
        with pytest.raises(NotImplementedError, match="input gradients"):
            low(a["upper_l"], x.clone(), None, None, None, None, body, a["R"], a["t"])
        if name != "upper_l":
            with pytest.raises(NotImplementedError, match="input gradients"):
                wl(x.clone(), h0, c0, h0, c0, body, a["R"], a["t"])
        with torch.no_grad():                                   # grad disabled: nothing is owed, nothing raises
            low(a["upper_l"], x.clone(), None, None, None, None, body, a["R"], a["t"])
    low(up.clone(), x.clone(), None, None, None, None, body, R, t)
    wl(x.clone(), h0, c0, h0, c0, body, R, t)
    torch.cuda.synchronize()
