"""GPU: Lower_Net's input gradients (d loss / d upper_l, d loss / d R, d loss / d t) against the float64 CPU oracle, the kernel behind
them (mmego_lower_inputs_backward) against float64 formulas, and what must NOT change for callers whose inputs are detached.

Bar for gradients: tests/test_input_grads_gpu.py's GRAD_BAR -- max abs error below 2e-4 of the largest entry of that gradient.  The fp32
oracle sits within 2.5e-5 of the float64 oracle on that scale for the three input gradients at these shapes (3.3e-6 for the parameter
gradients), so the bar leaves fp32 rounding a factor of 8 or more: a miss is a bug.
"""
import json
import os

import pytest
import torch

from conftest import GOLDEN, set_lstm_dropout
from oracle import geometry as geo
from oracle import nets as on
from oracle import train as ot
from step_helpers import entry_points as _entry_points

pytestmark = pytest.mark.gpu

GRAD_BAR = 2e-4
NEW_BUFFERS = ("pts_raw", "dR", "dt", "d_upper_l", "gcn.dup", "base.dy0")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _f64(v):
    return v.double().cpu()


def _rel_err(got, want):
    return float((got.double().cpu() - want).abs().max()), float(want.abs().max())


def test_lower_inputs_backward_against_float64(dev):
    """mmego_lower_inputs_backward alone: F in (1, 33, 512), N in (64, 128, 256) with P = 64 random distinct indices per frame, one
    frame's raw rows partly zero (they contribute p - t = -t), R perturbed by 1e-2 noise (not orthonormal), the gradient sources with the
    net's strides (6 and 128 for the points; 173 at column 128 and 45 for the joints).  One source and two; points-only, joints-only,
    both; dR / dt NULL; d upper_l NULL; accumulate onto random contents; a second run with equal bits."""
    from mmego_amd import hip
    gen = torch.Generator().manual_seed(61)
    V, P = 15, 64
    for F in (1, 33, 512):
        for N in (64, 128, 256):
            pts = torch.randn(F * N, 6, generator=gen)
            pts[N // 2:N] = 0.0                                   # (frame 0: zero-padded rows, selected like any other)
            idx = torch.stack([torch.randperm(N, generator=gen)[:P] for _ in range(F)]).contiguous()
            R = (geo.rot6d_imu(torch.randn(F, 6, generator=gen)) + 1e-2 * torch.randn(F, 3, 3, generator=gen)).contiguous()
            t = torch.randn(F, 3, generator=gen)
            ga, gb = torch.randn(F * P, 6, generator=gen), torch.randn(F * P, 128, generator=gen)
            up = torch.randn(F, V, 3, generator=gen)
            gja, gjb = torch.randn(F, 173, generator=gen), torch.randn(F, 45, generator=gen)
            d_pts = _f64(pts)[:, :3].view(F, N, 3).gather(1, idx.view(F, P, 1).expand(F, P, 3)) - _f64(t)[:, None, :]
            d_up = _f64(up) - _f64(t)[:, None, :]
            h = {k: v.to(dev) for k, v in dict(pts=pts, idx=idx, R=R, t=t, ga=ga, gb=gb, up=up, gja=gja, gjb=gjb).items()}
            gjv = h["gja"][:, 128:173]
            assert gjv.stride(0) == 173
            for two in (False, True):
                gp = (_f64(ga)[:, :3] + (_f64(gb)[:, :3] if two else 0)).view(F, P, 3)
                gj = (_f64(gja)[:, 128:173] + (_f64(gjb) if two else 0)).view(F, V, 3)
                for share in ("points", "joints", "both"):
                    use_p, use_j = share != "joints", share != "points"
                    want_R = torch.zeros(F, 3, 3, dtype=torch.float64)
                    s = torch.zeros(F, 3, dtype=torch.float64)
                    if use_p:
                        want_R += torch.einsum("fni,fnk->fik", gp, d_pts)
                        s += gp.sum(1)
                    if use_j:
                        want_R += torch.einsum("fvi,fvk->fik", gj, d_up)
                        s += gj.sum(1)
                    want_t = -torch.einsum("fik,fi->fk", _f64(R), s)
                    want_u = torch.einsum("fik,fvi->fvk", _f64(R), gj)

                    def run(acc, dR, dt, du):
                        hip.call("lower_inputs_backward", h["pts"] if use_p else None, 6, F, N, h["idx"] if use_p else None, P, h["R"], h["t"],
                                 h["ga"] if use_p else None, 6, h["gb"] if (use_p and two) else None, 128,
                                 h["up"] if use_j else None, V, gjv if use_j else None, 173, h["gjb"] if (use_j and two) else None, 45,
                                 acc, dR, dt, du)

                    dR, dt, du = torch.full((F, 3, 3), 7.0, device=dev), torch.full((F, 3), 7.0, device=dev), torch.full((F, V, 3), 7.0, device=dev)
                    run(0, dR, dt, du if use_j else None)
                    outs = [("dR", dR, want_R), ("dt", dt, want_t)] + ([("d_upper_l", du, want_u)] if use_j else [])
                    for name, got, want in outs:
                        err, scale = _rel_err(got, want)
                        print("lower_inputs_backward F=%d N=%d two=%d %s %s: %.3e at scale %.3e" % (F, N, two, share, name, err, scale))
                        assert err < GRAD_BAR * scale, (F, N, two, share, name, err, scale)
                    # accumulate: added to what dR / dt hold (d upper_l is written, never accumulated)
                    base_R, base_t = torch.randn(F, 3, 3, generator=gen).to(dev), torch.randn(F, 3, generator=gen).to(dev)
                    acc_R, acc_t, du_a = base_R.clone(), base_t.clone(), torch.full((F, V, 3), 3.0, device=dev)
                    run(1, acc_R, acc_t, du_a if use_j else None)
                    assert torch.equal(acc_R, base_R + dR) and torch.equal(acc_t, base_t + dt)
                    # a second run: the same bits
                    dR2, dt2, du2 = torch.empty_like(dR), torch.empty_like(dt), torch.empty_like(du)
                    run(0, dR2, dt2, du2 if use_j else None)
                    assert torch.equal(dR2, dR) and torch.equal(dt2, dt)
                    if use_j:
                        assert torch.equal(du_a, du) and torch.equal(du2, du)
                        # dR / dt NULL: only d upper_l is wanted -- same bits; d upper_l NULL: dR, dt with the same bits
                        du3 = torch.empty_like(du)
                        run(0, None, None, du3)
                        assert torch.equal(du3, du)
                        dR3, dt3 = torch.empty_like(dR), torch.empty_like(dt)
                        run(0, dR3, dt3, None)
                        assert torch.equal(dR3, dR) and torch.equal(dt3, dt)
    torch.cuda.synchronize()


# ---- LowerNet against the float64 oracle --------------------------------------------------------------------------------------------
B0, T0 = 4, 8
CASES = [  # (B, T, N, orthonormal, need_upper_l, need_R, need_t, padded)
    (B0, T0, 128, True, True, True, True, False),
    (B0, T0, 128, False, True, True, True, False),
    (B0, T0, 128, True, True, False, False, False),
    (B0, T0, 128, True, False, True, False, False),
    (B0, T0, 128, True, False, False, True, False),
    (B0, T0, 64, False, True, True, True, False),
    (B0, T0, 256, True, True, True, True, False),
    (3, 5, 128, False, True, True, True, False),          # 15 frames: ragged for every 4- and 64-frame partition
    (B0, T0, 128, False, True, True, True, True),
]


def _pair(dev, seed):
    """The oracle in float64 and the HIP net with the same weights, train mode, LSTM dropout off on both sides."""
    from mmego_amd import nets
    torch.manual_seed(seed)
    o = on.LowerNet(64).train()
    h = nets.LowerNet(64).to(dev).train()
    h.load_state_dict({k: v.to(dev) for k, v in o.state_dict().items()})
    set_lstm_dropout(o, 0.0)
    set_lstm_dropout(h, 0.0)
    h.lstm_dropout = 0
    h.differentiable_inputs = True
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
    up = torch.randn(B, T, 15, 3, generator=g)
    target = torch.randn(B, T, 8, 3, generator=g)
    return x, body, R, t, up, target


def _oracle_grads(o, x, body, R, t, up, target, idx):
    """float64 CPU oracle, all three inputs requiring grad -> (joints, d upper_l, dR, dt, {name: parameter gradient})."""
    ud, Rd, td = up.double().requires_grad_(), R.double().requires_grad_(), t.double().requires_grad_()
    for p in o.parameters():
        p.grad = None
    l = o(ud, x.double().clone(), None, None, None, None, body.double(), Rd, td, pin_select_idx=idx)[0]
    ot.l1_sum(l, target.double()).backward()
    return l.detach(), ud.grad, Rd.grad, td.grad, {k: (p.grad.clone() if p.grad is not None else None) for k, p in o.named_parameters()}


def _hip_grads(h, dev, x, body, R, t, up, target, need_u=True, need_R=True, need_t=True):
    uh = up.to(dev).requires_grad_(need_u)
    Rh, th = R.to(dev).requires_grad_(need_R), t.to(dev).requires_grad_(need_t)
    for p in h.parameters():
        p.grad = None
    l = h(uh, x.to(dev).clone(), None, None, None, None, body.to(dev), Rh, th)[0]
    (l - target.to(dev)).abs().sum().backward()
    torch.cuda.synchronize()
    return l.detach(), uh.grad, Rh.grad, th.grad, {k: p.grad.clone() for k, p in h.named_parameters()}, h.last_select_idx.clone().cpu()


_REFS = {}          # case -> (selection, oracle results): computed once, shared by the fused and the unfused run


@pytest.fixture(scope="module")
def pair(dev):
    o, h = _pair(dev, 13)
    return o, h, {k: v.clone() for k, v in o.state_dict().items()}


@pytest.mark.parametrize("fused", [True, False], ids=["gcn_fused", "gcn_unfused"])
def test_lower_input_gradients_against_oracle(dev, pair, fused):
    """Train mode, loss |l - target|.sum(), differentiable_inputs = True.  The HIP net runs first and hands its selection to the oracle
    (fp32 and float64 may order near-equal keys differently at the cut).  Cases: see CASES; the whole list with the fused ST-GCN training
    kernels and once more with the unfused forms (data_bn's input gradient comes from another kernel there)."""
    from mmego_amd import nets
    o, h, before = pair
    keep = nets._GCN_FUSED
    nets._GCN_FUSED = fused
    try:
        for i, case in enumerate(CASES):
            B, T, N, orth, need_u, need_R, need_t, padded = case
            h.load_state_dict({k: v.float().to(dev) for k, v in before.items()})      # (BatchNorm running statistics: every case from the same state)
            x, body, R, t, up, target = _batch(300 + i, B, T, N, orth, padded)
            lh, duh, dRh, dth, _, idx = _hip_grads(h, dev, x, body, R, t, up, target, need_u, need_R, need_t)
            assert h._gcn_was_fused == fused
            if case not in _REFS:
                o.load_state_dict(before)
                _REFS[case] = (idx, _oracle_grads(o, x, body, R, t, up, target, idx))
            idx0, (lo, duo, dRo, dto, _) = _REFS[case]
            assert torch.equal(idx, idx0)
            print("case", case, "fused", fused, "joints max err %.3e" % float((lh.double().cpu() - lo).abs().max()))
            assert torch.allclose(lh.cpu(), lo.float(), rtol=1e-4, atol=2e-5), (case, float((lh.double().cpu() - lo).abs().max()))
            for name, need, got, want, like in (("d_upper_l", need_u, duh, duo, up), ("dR", need_R, dRh, dRo, R), ("dt", need_t, dth, dto, t)):
                assert (got is not None) == need, (case, name)
                if need:
                    assert got.shape == like.shape and got.dtype == torch.float32, (case, name)
                    err, scale = _rel_err(got, want)
                    print("   %s max err %.3e at scale %.3e (%.2e of it)" % (name, err, scale, err / scale))
                    assert err < GRAD_BAR * scale, (case, name, err, scale)
    finally:
        nets._GCN_FUSED = keep


def test_lower_input_gradients_are_reproducible_and_leave_parameter_gradients_alone(dev, pair):
    """Two runs give the three gradients bit for bit (fixed-order reductions, no atomics), and asking for the input gradients does not
    change a bit of the parameter gradients; the parameter gradients of the case with all three inputs are inside the bar as well."""
    o, h, before = pair
    B, T, N = B0, T0, 128
    x, body, R, t, up, target = _batch(400, B, T, N, False, True)
    runs = []
    for need in (True, True, False):
        h.load_state_dict({k: v.float().to(dev) for k, v in before.items()})
        runs.append(_hip_grads(h, dev, x, body, R, t, up, target, need, need, need))
    (l0, du0, dR0, dt0, p0, i0), (l1, du1, dR1, dt1, p1, i1), (l2, du2, dR2, dt2, p2, i2) = runs
    assert torch.equal(l0, l1) and torch.equal(du0, du1) and torch.equal(dR0, dR1) and torch.equal(dt0, dt1)
    assert du2 is None and dR2 is None and dt2 is None and torch.equal(l0, l2)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
        assert torch.equal(p0[k], p2[k]), k                      # with / without requires_grad on the inputs
    assert min(float(v.abs().max()) for v in (du0, dR0, dt0)) > 0
    o.load_state_dict(before)
    _, _, _, _, po = _oracle_grads(o, x, body, R, t, up, target, i0)
    scale = max(float(v.abs().max()) for v in po.values() if v is not None)
    for k, v in po.items():
        want = v if v is not None else torch.zeros_like(dict(o.named_parameters())[k])
        err = float((p0[k].double().cpu() - want).abs().max())
        assert err < GRAD_BAR * scale, (k, err, scale)


def test_default_lower_step_is_unchanged(dev):
    """A StageStep("lower") without the new options launches exactly what it launched before Lower_Net had input gradients
    (tests/golden/lower_step_entry_points.json: the recorded entry points of StageStep("lower")._body, B=4, T=8, N=128, recorded head
    pose, written down on the commit before this feature) and keeps none of the new buffers."""
    from mmego_amd import nets
    from mmego_amd.train_step import StageStep
    B, T, N = 4, 8, 128
    torch.manual_seed(3)
    upper = nets.UpperNet().to(dev).eval()
    net = nets.LowerNet(64).to(dev).train()
    g = torch.Generator().manual_seed(4)
    xs = torch.randn(B, T, N, 6, generator=g).to(dev)
    tgt = torch.randn(B, T, 21, 3, generator=g).to(dev)
    body = (torch.randn(B, 20, 3, generator=g) * 0.3).to(dev)
    R = geo.rot6d_imu(torch.randn(B * T, 6, generator=g)).view(B, T, 3, 3).contiguous().to(dev)
    st = StageStep("lower", net, None, upper_frozen=upper, use_graph=False)
    st.bind(xs, None, body, tgt, R_gt=R)
    st.step()
    torch.cuda.synchronize()
    names = _entry_points(st._body)
    want = json.load(open(os.path.join(GOLDEN, "lower_step_entry_points.json")))
    assert names == want["entry_points"], [(i, a, b) for i, (a, b) in enumerate(zip(names, want["entry_points"])) if a != b][:5]
    assert getattr(net, "_ingrad", None) is None and st.upper_opt is None
    assert not any(net.arena("train").has(k) for k in NEW_BUFFERS)
    assert not any(upper.arena(a).has(k) for a in ("train", "eval") for k in ("dy_extra", "dl_sum"))
