"""GPU: global-norm gradient clipping inside the fused Adam step (FusedAdam(max_grad_norm=...), --clip_grad_norm).

Two launches: mmego_grad_sqnorm leaves one fp64 record per workgroup (the sum of its elements' squares, every product formed in fp64),
mmego_adam_step_clipped sums the records in its prologue and runs mmego_adam_step's update on g * cf,
    norm = sqrt(sum),  c = min(1, max_norm / (norm + 1e-6)) in double,  cf = (float)c,
or nothing at all when the norm is not finite.  The arithmetic is fixed, so the update tests are bit-exact: the second set of buffers is
advanced by the plain mmego_adam_step on torch's fp32 product g * cf, cf restated here from the norm the kernel reports.

Bars: the norm against float64 within (n + 4) * 2^-53 relative (the squares are exact in fp64: only the n - 1 additions, the host's own
sum and the root round); against torch.optim.Adam behind torch.nn.utils.clip_grad_norm_ atol 2e-7, the bar of
tests/test_hip_parity.py::test_fused_adam_matches_torch (torch forms norm and coefficient in fp32: a CPU restatement with the fp64 norm
stays within 1.2e-7 of it on this schedule, and the clipped and unclipped trajectories are 2e-5 to 1e-4 apart from step 2 on)."""
import glob
import math
import os
import re

import numpy as np
import pytest
import torch

from adam_helpers import ADAM, AdamSet as _Set, same_bits as _same_bits
from conftest import ROOT
from oracle import geometry as geo
from step_helpers import entry_points as _entry_points

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SENTINEL = -7.5
TRIP_FLOATS = 1024          # one workgroup's footprint per grid-stride trip: 256 lanes x one 16-byte load
UNROLL = 4                  # trips whose loads the kernel issues together (csrc/optim.hip GN_UNROLL)
MAX_NBLK = 1024             # the most records mmego_grad_norm_nblk returns (csrc/optim.hip GN_MAX_BLOCKS)
SECOND_TRIP_N = MAX_NBLK * TRIP_FLOATS + 4      # 1048580: the smallest n at which a workgroup (the first) takes a second trip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _nblk(n):
    from mmego_amd import hip
    return hip.lib().mmego_grad_norm_nblk(n)


def _records(dev, g, skip=None, pad=8):
    """mmego_grad_sqnorm on g -> (records, the sentinels behind them)."""
    from mmego_amd import hip
    n = g.numel()
    nb = _nblk(n)
    buf = torch.full((nb + pad,), SENTINEL, dtype=torch.float64, device=dev)
    hip.call("grad_sqnorm", g, n, skip, 0 if skip is None else skip.numel() // 2, buf, nb)
    torch.cuda.synchronize()
    return buf[:nb].clone(), buf[nb:].clone()


def _cf(norm, max_norm):
    """The clip factor as the kernel forms it: double arithmetic, one rounding to fp32."""
    c = max_norm / (norm + 1e-6)
    c = 1.0 if c > 1.0 else c
    return float(np.float32(c))


def _schedule(n, seed=5):
    """tests/test_hip_parity.py::test_fused_adam_matches_torch's gradients: randn * 10^(step - 3), five steps."""
    torch.manual_seed(seed)
    p0 = torch.randn(n)
    return p0, [torch.randn(n) * (10.0 ** (step - 3)) for step in range(1, 6)]


# ---- 1. the norm --------------------------------------------------------------------------------------------------------------------------
def test_second_trip_constant():
    """SECOND_TRIP_N from mmego_grad_norm_nblk and the per-trip footprint: the last n that one trip of all workgroups covers, plus 4."""
    assert _nblk(1 << 40) == MAX_NBLK and MAX_NBLK <= 2048
    assert _nblk(SECOND_TRIP_N) * TRIP_FLOATS == SECOND_TRIP_N - 4 and _nblk(SECOND_TRIP_N - 4) * TRIP_FLOATS >= SECOND_TRIP_N - 4
    assert [_nblk(n) for n in (4, 1020, 1024, 1028, 4104)] == [1, 1, 1, 2, 5]


# (beyond the issue's list: the sizes at which a lane first takes the unrolled loop -- 3 trips + 1 -- then the unrolled loop AND the
#  single-trip tail, then two unrolled rounds)
NORM_SIZES = [4, 1020, 1024, 1028, 4104, SECOND_TRIP_N + 12,
              (UNROLL - 1) * MAX_NBLK * TRIP_FLOATS + 4 + 12, UNROLL * MAX_NBLK * TRIP_FLOATS + 4 + 12, 2 * UNROLL * MAX_NBLK * TRIP_FLOATS + 16]


@pytest.mark.parametrize("n", NORM_SIZES)
def test_norm_against_float64(dev, n):
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(n % 9973))
    for scale in (1e-3, 1.0, 1e3, 3e20):
        if scale == 3e20 and n != 4104:
            continue                                  # (one case where the fp32 squares overflow)
        g = (g0 * scale).to(dev)
        want = float(g.cpu().double().pow(2).sum().sqrt())
        part, tail = _records(dev, g)
        got = float(part.cpu().sum().sqrt())
        rel = abs(got - want) / want
        print("grad norm n=%d scale %g: %.17g against %.17g, off by %.3e (bar %.3e)" % (n, scale, got, want, rel, (n + 4) * U))
        assert math.isfinite(got) and rel <= (n + 4) * U, (n, scale, got, want)
        assert bool((tail == SENTINEL).all())
        again, _ = _records(dev, g)
        assert torch.equal(part, again), (n, scale)
        if scale == 3e20:
            assert not bool(torch.isfinite(g * g).all())                      # (the fp32 squares do overflow)


# ---- 2. skip ranges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [1e30, float("nan")])
def test_skip_ranges(dev, fill):
    n = 4104
    skip = torch.tensor([0, 8, 1024, 2048, n - 4, n], dtype=torch.int64)
    inside = torch.zeros(n, dtype=torch.bool)
    for lo, hi in skip.view(-1, 2).tolist():
        inside[lo:hi] = True
    p0, grads = _schedule(n)
    g = grads[3].clone()
    rest = g.clone()
    rest[inside] = 0.0
    g[inside] = fill
    part, tail = _records(dev, g.to(dev), skip)
    zeroed, _ = _records(dev, rest.to(dev))
    assert torch.equal(part, zeroed) and bool((tail == SENTINEL).all())      # (adding 0.0 is exact: the same additions in the same order)
    want = float(rest.double().pow(2).sum().sqrt())
    assert abs(float(part.cpu().sum().sqrt()) - want) <= (n + 4) * U * want
    s = _Set(dev, p0)
    s.m.fill_(0.25), s.v.fill_(0.5)
    before = s.snapshot()
    s.step(g.to(dev), 1e-3, max_norm=1.0, skip=skip)
    after = s.snapshot()
    ins = inside.to(dev)
    for a, b in zip(before[:3], after[:3]):
        assert _same_bits(a[ins], b[ins])
        assert bool((a[~ins] != b[~ins]).all())
    assert bool(torch.isfinite(after[0]).all()) and s.stats[5].item() == 0 and s.stats[4].item() == 1 and s.state[0].item() == 1


# ---- 3. the update, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_update_equals_plain_step_on_the_scaled_gradient(dev, wd):
    n = 4096 + 8
    p0, grads = _schedule(n)
    a, b = _Set(dev, p0), _Set(dev, p0)
    norms = []
    for step, g in enumerate(grads, 1):
        g = g.to(dev)
        a.step(g, wd, max_norm=1.0)
        torch.cuda.synchronize()
        norm = a.stats[0].item()
        norms.append(norm)
        want = float(g.cpu().double().pow(2).sum().sqrt())
        assert abs(norm - want) <= (n + 4) * U * want
        cf = _cf(norm, 1.0)
        assert (cf < 1.0) == (step >= 2), (step, norm, cf)
        b.step(g * torch.tensor(cf, dtype=torch.float32, device=dev), wd)
        assert a.same_adam(b), (wd, step)
        assert a.ticket.item() == 0
    print("clip schedule norms:", " ".join("%.4g" % x for x in norms))
    assert 0.5 < norms[0] < 0.8 and 5e3 < norms[4] < 8e3
    st = a.stats.tolist()
    assert st[3] == 5 and st[4] == 4 and st[5] == 0 and st[0] == norms[4] and st[2] == max(norms)
    assert abs(st[1] - sum(norms)) <= 8 * U * sum(norms) and a.state[0].item() == 5


@pytest.mark.parametrize("max_norm", [1e30, float("inf")])
def test_threshold_out_of_reach_is_the_plain_step(dev, max_norm):
    n = 4096 + 8
    for wd in (0.0, 1e-3):
        p0, grads = _schedule(n)
        a, b = _Set(dev, p0), _Set(dev, p0)
        for step, g in enumerate(grads, 1):
            g = g.to(dev)
            a.step(g, wd, max_norm=max_norm)
            b.step(g, wd)
            assert a.same_adam(b), (wd, step)
        assert a.stats[4].item() == 0 and a.stats[3].item() == 5 and a.stats[5].item() == 0


# ---- 4. against torch ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_against_torch_clip_grad_norm_and_adam(dev, wd):
    n = 4096 + 8
    p0, grads = _schedule(n)
    ref_p = p0.clone().requires_grad_(True)
    free_p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref_p], lr=3e-5, weight_decay=wd)
    free = torch.optim.Adam([free_p], lr=3e-5, weight_decay=wd)
    a = _Set(dev, p0)
    for step, g in enumerate(grads, 1):
        ref_p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
        opt.step()
        free_p.grad = g.clone()
        free.step()
        a.step(g.to(dev), wd, max_norm=1.0)
        err = float((a.p.cpu() - ref_p.detach()).abs().max())
        apart = float((ref_p.detach() - free_p.detach()).abs().max())
        print("clipped adam wd %g step %d: %.3e from torch, clipped and unclipped torch %.3e apart" % (wd, step, err, apart))
        assert torch.allclose(a.p.cpu(), ref_p.detach(), rtol=0, atol=2e-7), (wd, step, err)
        if step >= 2:
            assert apart > 1e-5                                               # (a clip that does nothing would not pass)
    assert a.state[0].item() == 5.0 and a.ticket.item() == 0


# ---- 5. non-finite ------------------------------------------------------------------------------------------------------------------------
def test_non_finite_gradient_skips_the_step(dev):
    n = 4096 + 8
    p0, grads = _schedule(n)
    a, b = _Set(dev, p0), _Set(dev, p0)
    wd = 1e-3
    a.step(grads[2].to(dev), wd, max_norm=1.0)
    keep = a.snapshot()
    assert a.state[0].item() == 1
    for k, bad in enumerate((float("inf"), float("nan")), 1):
        g = grads[3].clone()
        g[1234] = bad
        a.step(g.to(dev), wd, max_norm=1.0)
        assert a.same_adam(keep), bad
        assert a.ticket.item() == 0 and a.stats[5].item() == k and a.stats[3].item() == 1 + k
        assert not math.isfinite(a.stats[0].item())
    a.step(grads[3].to(dev), wd, max_norm=1.0)
    torch.cuda.synchronize()
    assert a.state[0].item() == 2 and a.stats[5].item() == 2 and a.stats[3].item() == 4 and a.stats[4].item() == 2
    assert math.isfinite(a.stats[1].item()) and math.isfinite(a.stats[2].item())
    # the same two finite steps without the bad ones in between
    for i in (2, 3):
        b.step(grads[i].to(dev), wd, max_norm=1.0)
    assert a.same_adam(b)


# ---- 6. capture ---------------------------------------------------------------------------------------------------------------------------
def test_captured_pair_replays_as_three_eager_steps(dev):
    from mmego_amd import ops
    n = 4096 + 8
    p0, grads = _schedule(n)
    a, b = _Set(dev, p0), _Set(dev, p0)
    for g in grads[1:4]:
        a.step(g.to(dev), 1e-3, max_norm=1.0)
    torch.cuda.synchronize()
    gbuf = torch.zeros(n, device=dev)
    graph = torch.cuda.CUDAGraph()
    with ops.capture(graph):
        b.step(gbuf, 1e-3, max_norm=1.0)
    assert b.state[0].item() == 0                                             # (capturing executes nothing)
    for g in grads[1:4]:
        gbuf.copy_(g)
        graph.replay()
    assert a.same_adam(b) and torch.equal(a.stats, b.stats) and b.state[0].item() == 3 and b.stats[4].item() == 3


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    from mmego_amd import hip
    n = 4104
    nb = _nblk(n)
    buf = {k: torch.full((n + 8,), SENTINEL, device=dev) for k in "pgmv"}
    part = torch.full((nb + 8,), SENTINEL, dtype=torch.float64, device=dev)
    state = torch.zeros(3, dtype=torch.float64, device=dev)
    stats = torch.zeros(8, dtype=torch.float64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    p, g, m, v = (buf[k] for k in "pgmv")

    def norm(g_, n_, npart):
        hip.call("grad_sqnorm", g_, n_, None, 0, part, npart)

    def update(p_, g_, n_, npart, max_norm):
        hip.call("adam_step_clipped", p_, g_, m, v, n_, state, *ADAM, 1e-3, None, 0, ticket, part, npart, max_norm, stats)

    bad = [lambda: norm(g, n - 2, nb), lambda: norm(g[1:], n, nb), lambda: norm(g, n, nb + 1), lambda: norm(g, n, nb - 1),
           lambda: update(p, g, n - 2, nb, 1.0), lambda: update(p[1:], g, n, nb, 1.0), lambda: update(p, g[1:], n, nb, 1.0),
           lambda: update(p, g, n, nb + 1, 1.0), lambda: update(p, g, n, nb - 1, 1.0),
           lambda: update(p, g, n, nb, 0.0), lambda: update(p, g, n, nb, -1.0), lambda: update(p, g, n, nb, float("nan"))]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError, match="bad argument"):
            call()
    torch.cuda.synchronize()
    for t in list(buf.values()) + [part]:
        assert bool((t == SENTINEL).all())
    assert not bool(state.any()) and not bool(stats.any()) and ticket.item() == 0
    skip = torch.tensor([0, 6], dtype=torch.int64)                            # (a range that is no multiple of 4: as mmego_adam_step)
    with pytest.raises(RuntimeError, match="bad argument"):
        hip.call("grad_sqnorm", g, n, skip, 1, part, nb)
    update(p, g, n, nb, float("inf"))                                         # (+inf is a threshold)
    torch.cuda.synchronize()


# ---- 8. FusedAdam -------------------------------------------------------------------------------------------------------------------------
def test_fused_adam_launches_and_never_trained_ranges(dev):
    from mmego_amd import nets
    from mmego_amd.params import FusedAdam
    torch.manual_seed(7)
    net = nets.IMUNet(15, 9, 32, 2, True, 0).to(dev).train()
    flat = net.flat().ensure()
    plain = FusedAdam(net.flat(), lr=1e-3, weight_decay=1e-3)
    assert _entry_points(plain.step) == ["adam_step"]
    assert plain._part is None and plain._stats is None and plain.grad_stats() is None
    opt = FusedAdam(net.flat(), lr=1e-3, weight_decay=1e-3, max_grad_norm=0.5)
    assert _entry_points(opt.step) == ["grad_sqnorm", "adam_step_clipped"]
    dead = torch.zeros(flat.flat_p.numel(), dtype=torch.bool, device=dev)
    for prm, off in zip(flat.params, flat.offsets):
        if any(prm is q for q in net.never_trained()):
            dead[off:off + (prm.numel() + 3) // 4 * 4] = True
    assert bool(dead.any()) and not bool(dead.all())
    flat.flat_g.copy_(torch.randn(flat.flat_g.numel(), generator=torch.Generator().manual_seed(8)))
    want = float(flat.flat_g[~dead].double().pow(2).sum().sqrt())
    flat.flat_g[dead] = float("nan")                                          # (grad=None for torch: neither in the norm nor updated)
    before = flat.flat_p.clone()
    opt.step()
    torch.cuda.synchronize()
    s = opt.grad_stats()
    assert s["steps"] == 1 and s["clipped"] == 1 and s["skipped"] == 0 and abs(s["last"] - want) <= (flat.flat_g.numel() + 4) * U * want
    assert s["mean"] == s["last"] == s["max"]
    assert _same_bits(flat.flat_p[dead], before[dead]) and not bool(opt.m[dead].any()) and not bool(opt.v[dead].any())
    live = ~dead
    for prm, off in zip(flat.params, flat.offsets):                           # (alignment padding between tensors has zero gradient)
        live[off + prm.numel():off + (prm.numel() + 3) // 4 * 4] = False
    assert bool((flat.flat_p[live] != before[live]).all())
    for k, prm in net.named_parameters():
        if k.startswith("fc3."):
            assert bool(dead[flat.offsets[[id(q) for q in flat.params].index(id(prm))]])
    opt.reset_grad_stats()
    assert opt.grad_stats()["steps"] == 0
    sd = opt.state_dict()
    assert sd["max_grad_norm"] == 0.5
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam(net.flat(), max_grad_norm=0.0)


# ---- 9. the training steps, end to end ----------------------------------------------------------------------------------------------------
class _HostClip:
    """What FusedAdam(max_grad_norm=c) must equal: read the norm, scale the flat gradient by cf with torch's fp32 multiply, take the
    plain step."""

    def __init__(self, opt, c):
        self.opt, self.c, self.clipped = opt, c, 0
        self.m = self.v = None

    def step(self):
        from mmego_amd import hip
        f = self.opt._ensure()
        skip = self.opt._skip_ranges(f)
        n = f.flat_g.numel()
        part = torch.zeros(_nblk(n), dtype=torch.float64, device=f.flat_g.device)
        hip.call("grad_sqnorm", f.flat_g, n, skip if skip is not False else None, skip.numel() // 2 if skip is not False else 0, part,
                 part.numel())
        # (the records summed as the kernel's prologue sums them: lane j takes j, j + 256, ...; butterfly; waves in order)
        norm = math.sqrt(_prologue_sum(part.cpu()))
        cf = _cf(norm, self.c)
        self.clipped += cf < 1.0
        f.flat_g.mul_(torch.tensor(cf, dtype=torch.float32, device=f.flat_g.device))
        self.opt.step()
        self.m, self.v = self.opt.m, self.opt.v


def _prologue_sum(part):
    """The fixed order of the clipped step's prologue (adam_step_kernel, CLIP) over the records, in numpy float64."""
    x = np.zeros(256 * ((part.numel() + 255) // 256))
    x[:part.numel()] = part.numpy()
    lanes = np.zeros(256)
    for row in x.reshape(-1, 256):
        lanes = lanes + row
    w = lanes.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ o]
    return float(((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


# The threshold of these tests is half the FIRST step's norm and all three steps have to be clipped.  On random targets a fresh IMU_Net's
# gradient norm falls by a factor of three per step at stage 1's learning rate 1e-4 (measured: 18183, 6193, 1186), below that threshold
# by the second step; at 1e-6 the weights still move by hundreds of ulps per step and the norm stays where it started.
IMU_LR = 1e-6


def _upper_setup(dev):
    from mmego_amd import nets
    B, T, N = 2, 4, 128
    torch.manual_seed(41)
    sd = {k: v.clone() for k, v in nets.UpperNet().state_dict().items()}
    sd_imu = {k: v.clone() for k, v in nets.IMUNet(15, 9, 512, 2, True, 0).state_dict().items()}
    g = torch.Generator().manual_seed(42)
    batch = [v.to(dev) for v in (torch.randn(B, T, N, 6, generator=g), torch.randn(B, T, 20, 15, generator=g),
                                 torch.randn(B, 20, 3, generator=g) * 0.3, torch.randn(B, T, 21, 3, generator=g))]
    R = geo.rot6d_imu(torch.randn(B * T, 6, generator=g)).view(B, T, 3, 3).contiguous().to(dev)
    return sd, sd_imu, batch, R


def _make_upper(dev, sd, sd_imu, batch, R, use_graph, finetune, clip):
    from mmego_amd import nets
    from mmego_amd.train_step import StageStep
    hup = nets.UpperNet()
    hup.load_state_dict(sd)
    hup = hup.to(dev).train()
    hup.lstm_dropout = 0.0
    himu = None
    if finetune:
        himu = nets.IMUNet(15, 9, 512, 2, True, 0)
        himu.load_state_dict(sd_imu)
        himu = himu.to(dev).train()
    st = StageStep("upper", hup, himu, lr=3e-5, use_graph=use_graph, finetune_imu=finetune, imu_lr=IMU_LR, clip_grad_norm=clip)
    st.bind(*batch, R_gt=None if finetune else R)
    return st


def _make_imu(dev, sd_imu, batch, R, use_graph, clip):
    from mmego_amd import nets
    from mmego_amd.train_step import ImuStep
    net = nets.IMUNet(15, 9, 512, 2, True, 0)
    net.load_state_dict(sd_imu)
    net = net.to(dev).train()
    st = ImuStep(net, lr=IMU_LR, use_graph=use_graph, clip_grad_norm=clip)
    st.bind(batch[1], R, batch[3])
    return st


def _opts(st):
    return [(n, getattr(st, n)) for n in ("opt", "imu_opt") if getattr(st, n, None) is not None]


def _clipped_step_equals_host_clip(make):
    probe = make(float("inf"))
    probe.step()
    torch.cuda.synchronize()
    first = [o.grad_stats() for _, o in _opts(probe)]
    assert all(s["steps"] == 1 and s["clipped"] == 0 and s["skipped"] == 0 and s["last"] > 0 for s in first)
    c = 0.5 * min(s["last"] for s in first)
    a, b = make(c), make(None)
    wraps = []
    for name, o in _opts(b):
        assert o.max_grad_norm is None
        wraps.append(_HostClip(o, c))
        setattr(b, name, wraps[-1])
    for step in range(3):
        la, lb = a.step().clone(), b.step().clone()
        torch.cuda.synchronize()
        assert torch.equal(la, lb), step
        for (name, oa), w in zip(_opts(a), wraps):
            fa, fb = oa.flat, w.opt.flat
            assert _same_bits(fa.flat_p, fb.flat_p), (step, name)
            assert _same_bits(oa.m, w.m) and _same_bits(oa.v, w.v) and torch.equal(oa.state, w.opt.state), (step, name)
    for (name, oa), w in zip(_opts(a), wraps):
        s = oa.grad_stats()
        print("clipped step %s: norms mean %.6g max %.6g, threshold %.6g, clipped %d/%d" % (name, s["mean"], s["max"], c, s["clipped"], s["steps"]))
        assert s["clipped"] == 3 and s["steps"] == 3 and s["skipped"] == 0 and w.clipped == 3, (name, s)


@pytest.mark.parametrize("use_graph", [False, True])
def test_upper_stage_step_clips_bit_exactly(dev, use_graph):
    sd, sd_imu, batch, R = _upper_setup(dev)
    _clipped_step_equals_host_clip(lambda clip: _make_upper(dev, sd, sd_imu, batch, R, use_graph, False, clip))


def test_imu_step_clips_bit_exactly(dev):
    sd, sd_imu, batch, R = _upper_setup(dev)
    _clipped_step_equals_host_clip(lambda clip: _make_imu(dev, sd_imu, batch, R, True, clip))


def test_finetune_imu_stage_clips_each_net_by_its_own_norm(dev):
    sd, sd_imu, batch, R = _upper_setup(dev)
    _clipped_step_equals_host_clip(lambda clip: _make_upper(dev, sd, sd_imu, batch, R, True, True, clip))


# ---- 10. the command line -----------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^Grad norm \(IMU_Net\): mean (\S+) max (\S+) clipped (\d+)/(\d+) skipped (\d+)$", re.M)


def _ckpt(out_dir, idx, epoch):
    f = [f for f in glob.glob(os.path.join(out_dir, "model", str(idx), "epoch%d_*.pth" % epoch)) if not f.endswith(".train_state.pth")]
    assert len(f) == 1, f
    return f[0]


def _equal_ckpt(a, b):
    sa, sb = torch.load(a, map_location="cpu"), torch.load(b, map_location="cpu")
    assert sa.keys() == sb.keys()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.fixture(scope="module")
def cli_tree(tmp_path_factory):
    """The synthetic tree of tests/test_cli_gpu.py, ONE stage-1 epoch with `--clip_grad_norm inf` and one with X = half the mean norm
    that run reports (below the mean: at least one step is clipped); the two tests below share them."""
    from test_cli_gpu import _make_dataset, _run
    tmp = tmp_path_factory.mktemp("clip_grad_norm_cli")
    data = str(tmp / "Sample_data")
    _make_dataset(data, np.random.default_rng(1))
    out_dir = str(tmp / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    base = ["--train", "--network", "IMU_Net", "--data_root", data, "--batch_size", "4", "--device", "cuda:0", "--seed", "0"]
    out = _run(base + ["--clip_grad_norm", "inf", "--epochs", "1", "--log_dir", "9160"], env)
    seen = LINE.findall(out)
    assert len(seen) == 1, out[-2000:]
    mean, top, clipped, steps, skipped = float(seen[0][0]), float(seen[0][1]), *map(int, seen[0][2:])
    assert clipped == 0 and skipped == 0 and steps > 0 and 0 < mean <= top
    x = repr(0.5 * mean)
    out = _run(base + ["--clip_grad_norm", x, "--epochs", "1", "--log_dir", "9161"], env)
    seen = LINE.findall(out)
    assert len(seen) == 1 and int(seen[0][2]) >= 1 and int(seen[0][3]) == steps and int(seen[0][4]) == 0, out[-2000:]
    return dict(out_dir=out_dir, env=env, base=base, run=_run, x=x)


def test_cli_stage1_clipping_is_reproducible_and_live(cli_tree):
    """--train --network IMU_Net --clip_grad_norm X --epochs 1 --seed 0 twice: equal checkpoints; without the flag: another one, no
    report line, and the checkpoint of the `inf` run (which measures and changes nothing)."""
    c = cli_tree
    c["run"](c["base"] + ["--clip_grad_norm", c["x"], "--epochs", "1", "--log_dir", "9162"], c["env"])
    out = c["run"](c["base"] + ["--epochs", "1", "--log_dir", "9163"], c["env"])
    assert "Grad norm" not in out
    first = _ckpt(c["out_dir"], 9161, 0)
    assert _equal_ckpt(first, _ckpt(c["out_dir"], 9162, 0))
    assert not _equal_ckpt(first, _ckpt(c["out_dir"], 9163, 0))
    assert _equal_ckpt(_ckpt(c["out_dir"], 9160, 0), _ckpt(c["out_dir"], 9163, 0))
    assert all(bool(torch.isfinite(v).all()) for v in torch.load(first, map_location="cpu").values())


def test_cli_stage1_clipping_resumes_without_the_flag(cli_tree):
    """One epoch plus --resume WITHOUT --clip_grad_norm equals two epochs with it, bit for bit: the optimizer state carries the threshold."""
    c = cli_tree
    out = c["run"](c["base"] + ["--clip_grad_norm", c["x"], "--epochs", "2", "--log_dir", "9164"], c["env"])
    assert len(LINE.findall(out)) == 2
    out = c["run"](c["base"] + ["--epochs", "2", "--log_dir", "9165", "--resume", _ckpt(c["out_dir"], 9161, 0)], c["env"])
    assert "resumed from" in out and "epoch: 2" in out and "epoch: 1\n" not in out
    assert len(LINE.findall(out)) == 1                                       # (the resumed run clips, so it reports)
    a, b = _ckpt(c["out_dir"], 9164, 1), _ckpt(c["out_dir"], 9165, 1)
    assert _equal_ckpt(a, b)
    ta = torch.load(a[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)
    tb = torch.load(b[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)
    assert torch.equal(ta["optimizer"]["m"], tb["optimizer"]["m"]) and torch.equal(ta["optimizer"]["state"], tb["optimizer"]["state"])
    assert ta["optimizer"]["max_grad_norm"] == tb["optimizer"]["max_grad_norm"] == float(c["x"])
