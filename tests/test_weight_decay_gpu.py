"""GPU: the fused Adam step with a decay mask and the decoupled (AdamW) form (csrc/optim.hip: mmego_adam_step_decay), FusedAdam's
decoupled / no_decay, the step engines' options of those names and `main.py --train --weight_decay ... --decay_mode adamw --no_decay_1d`.

Sizes as tests/test_ema_gpu.py: 4 floats (one lane), 1028 (257 float4: five mask words, one bit used in the last, a partial workgroup),
2 097 156 (exactly one lane takes a second grid-stride trip).  Masks (tests/decay_helpers.py): all set, all clear, seeded runs of 1..70
float4 alternating set and clear, only the last float4 set.  Forms: the four (ema, clip) forms of test_lr_schedule_gpu.FORMS, unscheduled
and under that file's cosine schedule.  Every comparison is on bit patterns unless a bound is named.

The decay against float64 (test 4): the kernel's dw is (float)(lr * weight_decay) by definition, and p' = fmaf(-dw, p, p) rounds the exact
p - dw p once, so against the float64 value of p - dw p AT THAT dw the bar is 0.5 ulp_fp32 (1 + 2^-20) per element (the 2^-20 pays for
the float64 evaluation).  The figure against the unrounded double product lr * weight_decay is printed beside it: the rounding of dw to
fp32 moves p' by at most 2^-24 dw |p|, far below an ulp, but is not part of what one fmaf rounds.

Against torch.optim.AdamW in float64 (tests 8, 10): the plain step (weight_decay 0) is measured against float64 torch.optim.Adam on the
same inputs first, worst error in units of ulp_fp32(|p|); the decoupled step may exceed that figure by one ulp per step taken."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from adam_helpers import ADAM, LR, grads as _seeded, same_bits as _same_bits
from conftest import ROOT
from decay_helpers import DecaySet as _Set, device_mask as _mask, ulp32 as _ulp32, worst_ulp as _worst_ulp
from step_helpers import entry_points as _entry_points
from test_lr_schedule_gpu import FORMS, KINDS, SENTINEL, SIZES, STEPS, _max_norm

pytestmark = pytest.mark.gpu

MASKS = ["set", "clear", "runs", "last"]
WD = 1e-3
EXACT_LR, EXACT_WD = 2.0 ** -15, 2.0 ** -3                                # dw = 2^-18: p - dw p is exact in float64 for fp32 p
_figures = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _cosine():
    from mmego_amd import hip
    return hip.LrSchedule(**KINDS["cosine"][0])


def _grads(dev, n):
    return _seeded(dev, n, STEPS)


def _old_step(s, g, wd, sched, decay, c, **kw):
    if sched is None:
        s.step(g, wd, decay=decay, max_norm=c, **kw)
    else:
        s.sched_step(g, wd, sched, decay=decay, max_norm=c, **kw)


def _all(s):
    """p, m, v, ema, stats and the whole state."""
    return s.tensors() + (s.state,)


# ---- 1. the new entry point without its option is the old step -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scheduled", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_without_its_option_the_entry_point_is_the_old_step(dev, n, scheduled):
    p0, grads = _grads(dev, n)
    sched = _cosine() if scheduled else None
    words = 4 if scheduled else 3
    for decay, clip in FORMS:
        c = _max_norm(clip, grads)
        for mask in (None, _mask(dev, n, "set")[0]):
            a, b = _Set(dev, p0, words), _Set(dev, p0, words)
            for t, g in enumerate(grads, 1):
                a.decay_step(g, WD, mask=mask, decoupled=False, sched=sched, decay=decay, max_norm=c)
                _old_step(b, g, WD, sched, decay, c)
                torch.cuda.synchronize()
                assert all(_same_bits(x, y) for x, y in zip(_all(a), _all(b))), (decay, clip, mask is None, t)
                assert a.state[0].item() == t and a.ticket.item() == 0
            assert not _same_bits(a.p, p0)


# ---- 2. a mask selects between two old steps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheduled", [False, True])
@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("n", SIZES)
def test_a_mask_selects_between_two_old_steps(dev, n, name, scheduled):
    p0, grads = _grads(dev, n)
    sched = _cosine() if scheduled else None
    words = 4 if scheduled else 3
    mask, sel = _mask(dev, n, name)
    wd = 0.05                                                               # (large enough that the two old steps part in the first step)
    for decay, clip in FORMS:
        c = _max_norm(clip, grads)
        a, b, z = _Set(dev, p0, words), _Set(dev, p0, words), _Set(dev, p0, words)
        for t, g in enumerate(grads, 1):
            a.decay_step(g, wd, mask=mask, decoupled=False, sched=sched, decay=decay, max_norm=c)
            _old_step(b, g, wd, sched, decay, c)
            _old_step(z, g, 0.0, sched, decay, c)
            torch.cuda.synchronize()
            for x, with_, without in zip(a.tensors()[:4], b.tensors()[:4], z.tensors()[:4]):
                assert _same_bits(x, torch.where(sel, with_, without)), (name, decay, clip, t)
            assert _same_bits(a.state, b.state) and _same_bits(a.stats, b.stats) and _same_bits(a.state, z.state)
        if name in ("runs", "last"):
            assert not _same_bits(b.p[sel], z.p[sel])                       # (the mask decided something)


# ---- 3. the decoupled step is a pre-scaled old step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("n", SIZES)
def test_the_decoupled_step_is_a_pre_scaled_old_step(dev, n, name):
    """lr = 2^-15, wd = 2^-3: dw = 2^-18 and p - dw p is exact in float64, so its single rounding to fp32 is what fmaf gives."""
    p0, grads = _grads(dev, n)
    mask, sel = _mask(dev, n, name)
    for decay, clip in FORMS:
        c = _max_norm(clip, grads)
        a, b = _Set(dev, p0), _Set(dev, p0)
        for t, g in enumerate(grads, 1):
            p64 = b.p.double()
            b.p.copy_(torch.where(sel, (p64 - 2.0 ** -18 * p64).float(), b.p))
            b.step(g, 0.0, decay=decay, max_norm=c, lr=EXACT_LR)
            a.decay_step(g, EXACT_WD, mask=mask, decoupled=True, decay=decay, max_norm=c, lr=EXACT_LR)
            torch.cuda.synchronize()
            assert all(_same_bits(x, y) for x, y in zip(_all(a), _all(b))), (name, decay, clip, t)
        if name != "clear":
            z = _Set(dev, p0)
            z.step(grads[0], 0.0, lr=EXACT_LR)
            y = _Set(dev, p0)
            y.decay_step(grads[0], EXACT_WD, mask=mask, decoupled=True, lr=EXACT_LR)
            assert not _same_bits(y.p[sel], z.p[sel])                       # (and it decays)


# ---- 4. the decay alone, general dw, against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr,wd", [(3e-5, 1e-2), (1e-4, 5e-2)])
def test_the_decay_alone_against_float64(dev, lr, wd):
    worst = worst_unrounded = 0.0
    for n in SIZES:
        p0, _ = _grads(dev, n)
        mask, sel = _mask(dev, n, "runs")
        a = _Set(dev, p0)
        a.decay_step(torch.zeros(n, device=dev), wd, mask=mask, decoupled=True, lr=lr)       # zero gradient and moments: the Adam term is 0
        torch.cuda.synchronize()
        assert _same_bits(a.p[~sel], p0[~sel]) and not bool(a.m.any()) and not bool(a.v.any())
        p64 = p0.double()[sel]
        for key, dw64 in (("rounded", float(np.float32(lr * wd))), ("unrounded", lr * wd)):
            want = p64 - dw64 * p64
            ratio = float(((a.p[sel].double() - want).abs() / _ulp32(want)).max()) if p64.numel() else 0.0
            if key == "rounded":
                worst = max(worst, ratio)
            else:
                worst_unrounded = max(worst_unrounded, ratio)
    print("lr %g wd %g: worst |p' - (p64 - dw p64)| = %.9f ulp_fp32 at dw = (float)(lr wd), %.9f at the double product"
          % (lr, wd, worst, worst_unrounded))
    _figures["decay_alone_%g_%g" % (lr, wd)] = (worst, worst_unrounded)
    assert worst <= 0.5 * (1.0 + 2.0 ** -20)


# ---- 5. scheduled ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_the_scheduled_decoupled_step_is_the_decoupled_step_at_its_rate(dev, n):
    p0, grads = _grads(dev, n)
    sched = _cosine()
    mask, _ = _mask(dev, n, "runs")
    for decay, clip in FORMS:
        c = _max_norm(clip, grads)
        a, b, u = _Set(dev, p0, 4), _Set(dev, p0, 3), _Set(dev, p0, 4)
        rates = set()
        for t, g in enumerate(grads, 1):
            a.decay_step(g, 0.05, mask=mask, decoupled=True, sched=sched, decay=decay, max_norm=c)
            u.sched_step(g, 0.0, sched, decay=decay, max_norm=c)           # (the undecayed run: the same rates)
            rate = a.state[3].item()
            rates.add(rate)
            b.decay_step(g, 0.05, mask=mask, decoupled=True, decay=decay, max_norm=c, lr=rate)
            assert a.same(b), (decay, clip, t)
            assert _same_bits(a.state, u.state)
        assert len(rates) >= 5 and not _same_bits(a.p, u.p)


# ---- 6. skipped steps and skip ranges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_skipped_steps_and_skip_ranges_do_not_decay(dev, n):
    p0, grads = _grads(dev, n)
    mask, _ = _mask(dev, n, "runs")
    sched = _cosine()
    a = _Set(dev, p0, 4)
    a.decay_step(grads[0], 0.05, mask=mask, decoupled=True, sched=sched, decay=0.9, max_norm=1.0)
    keep = a.snapshot(ema=True)
    g = grads[1].clone()
    g[n - 3] = float("nan")
    a.decay_step(g, 0.05, mask=mask, decoupled=True, sched=sched, decay=0.9, max_norm=1.0)
    for x, y in zip(a.snapshot(ema=True), keep):
        assert _same_bits(x, y)
    assert a.stats[5].item() == 1 and a.ticket.item() == 0 and a.state[0].item() == 1
    if n >= 1028:                                                           # a skip range never changes, whatever its bit
        skip = torch.tensor([8, 272], dtype=torch.int64)
        inside = torch.zeros(n, dtype=torch.bool, device=dev)
        inside[8:272] = True
        for decoupled in (False, True):
            for m_ in (None, mask):
                b = _Set(dev, p0)
                for g in grads[:2]:
                    b.decay_step(g, 0.05, mask=m_, decoupled=decoupled, decay=0.9, skip=skip)
                torch.cuda.synchronize()
                assert _same_bits(b.p[inside], p0[inside]) and _same_bits(b.ema[inside], p0[inside])
                assert not bool(b.m[inside].any()) and not bool(b.v[inside].any())
                # (outside it the update ran: nearly everything moved -- two steps of opposite sign may bring an element back exactly)
                assert float((b.p[~inside] != p0[~inside]).float().mean()) > 0.99 and bool((b.m[~inside] != 0).all())


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, "half"])
def test_one_captured_launch_of_the_scheduled_decoupled_form(dev, clip):
    from mmego_amd import ops
    n = SIZES[1]
    p0, grads = _grads(dev, n)
    sched = _cosine()
    mask, _ = _mask(dev, n, "runs")
    c = _max_norm(clip, grads)
    a, b = _Set(dev, p0, 4), _Set(dev, p0, 4)
    for g in grads:
        a.decay_step(g, 0.05, mask=mask, decoupled=True, sched=sched, decay=0.9, max_norm=c)
    torch.cuda.synchronize()
    gbuf = torch.zeros(n, device=dev)
    graph = torch.cuda.CUDAGraph()
    with ops.capture(graph):
        b.decay_step(gbuf, 0.05, mask=mask, decoupled=True, sched=sched, decay=0.9, max_norm=c)
    torch.cuda.synchronize()
    assert not bool(b.state.any()) and _same_bits(b.p, p0)                  # (capturing executes nothing)
    for g in grads:
        gbuf.copy_(g)
        graph.replay()
    assert a.same(b) and _same_bits(a.state, b.state) and b.state[0].item() == STEPS


# ---- 8. against torch.optim.AdamW in float64 -------------------------------------------------------------------------------------------------------
def _adam64(p0, grads, sel, lr, wd):
    """torch.optim.AdamW in float64 on the CPU, two groups: the elements of ``sel`` decay at ``wd``, the others do not."""
    sel = sel.cpu()
    with_, without = torch.nn.Parameter(p0.double().cpu()[sel]), torch.nn.Parameter(p0.double().cpu()[~sel])
    groups = [dict(params=[q], weight_decay=w) for q, w in ((with_, wd), (without, 0.0)) if q.numel()]
    opt = torch.optim.AdamW(groups, lr=lr, betas=ADAM[1:3], eps=ADAM[3])
    for g in grads:
        g = g.double().cpu()
        with_.grad, without.grad = g[sel], g[~sel]
        opt.step()
    out = torch.empty(p0.numel(), dtype=torch.float64)
    out[sel], out[~sel] = with_.detach(), without.detach()
    return out


def test_against_adamw_in_float64(dev):
    steps, wd = 3, 1e-2
    plain = decoupled = 0.0
    for n in SIZES[:2]:
        p0, grads = _grads(dev, n)
        mask, sel = _mask(dev, n, "runs")
        z, a = _Set(dev, p0), _Set(dev, p0)
        for g in grads[:steps]:
            z.step(g, 0.0)
            a.decay_step(g, wd, mask=mask, decoupled=True)
        torch.cuda.synchronize()
        # (AdamW at weight_decay 0 is torch.optim.Adam: the plain step's own error on these inputs)
        plain = max(plain, _worst_ulp(z.p, _adam64(p0, grads[:steps], sel, LR, 0.0)))
        decoupled = max(decoupled, _worst_ulp(a.p, _adam64(p0, grads[:steps], sel, LR, wd)))
    print("against float64, %d steps: plain step %.4f ulp_fp32(|p|), decoupled step at weight_decay %g %.4f" % (steps, plain, wd, decoupled))
    _figures["adamw"] = (plain, decoupled)
    assert decoupled <= plain + steps


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    import ctypes
    from mmego_amd import hip
    n = 1028
    buf = {k: torch.full((n + 8,), SENTINEL, device=dev) for k in "pgmv"}
    state8 = torch.zeros(8, dtype=torch.float64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    mask16 = torch.full((16,), -1, dtype=torch.int32, device=dev)
    nan, inf = float("nan"), float("inf")
    good = dict(wd=WD, mask=mask16, decoupled=1, sched=None, state=state8[:3])

    def args(**kw):
        a = dict(good, **kw)
        return (buf["p"], buf["g"], buf["m"], buf["v"], n, a["state"], *ADAM, a["wd"], None, 0, ticket, None, 0, 0.0, None, None, 0.0,
                a["sched"], a["mask"], a["decoupled"])

    bad = [dict(mask=mask16[1:]), dict(wd=-1e-3), dict(wd=nan), dict(wd=inf), dict(wd=-inf), dict(decoupled=2), dict(decoupled=-1)]
    for kw in bad:
        for extra in (dict(), dict(sched=_cosine(), state=state8[:4]), dict(decoupled=0) if "decoupled" not in kw else dict()):
            with pytest.raises(RuntimeError, match="bad argument"):
                hip.call("adam_step_decay", *args(**dict(extra, **kw)))
    rc = hip.lib().mmego_adam_step_decay(hip.stream_handle(), *[hip._conv(v) for v in args(decoupled=7)])
    assert rc != 0                                                           # (the return code itself)
    s = hip.LrSchedule(kind=9)                                              # what mmego_adam_step_sched refuses is refused here
    assert hip.lib().mmego_adam_step_decay(hip.stream_handle(), *[hip._conv(v) for v in args(sched=ctypes.addressof(s), state=state8[:4])]) != 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in buf.values())
    assert not bool(state8.any()) and ticket.item() == 0 and bool((mask16 == -1).all())


# ---- 10. FusedAdam ---------------------------------------------------------------------------------------------------------------------------------
def _fill(flat, seed):
    flat.flat_g.copy_(0.1 * torch.randn(flat.flat_g.numel(), generator=torch.Generator().manual_seed(seed)))


def test_fused_adam_decoupled_without_decay_for_1d(dev):
    from mmego_amd import nets
    from mmego_amd.params import FusedAdam
    torch.manual_seed(7)
    net = nets.UpperNet().to(dev).train()
    flat = net.flat().ensure()
    start = flat.flat_p.clone()
    steps, kw = 3, dict(lr=1e-3, weight_decay=1e-2)
    opt = FusedAdam(net.flat(), decoupled=True, no_decay="1d", **kw)
    one_d = {k for k, p in net.named_parameters() if p.dim() <= 1}
    assert set(opt.no_decay) == one_d and 0 < len(one_d) < len(flat.params)
    assert _entry_points(opt.step) == ["adam_step_decay"]
    assert _entry_points(FusedAdam(net.flat(), max_grad_norm=1.0, no_decay="1d", **kw).step) == ["grad_sqnorm", "adam_step_decay"]
    assert _entry_points(FusedAdam(net.flat(), **kw).step) == ["adam_step"]                    # (neither option: today's call)
    sel = torch.zeros(flat.flat_p.numel(), dtype=torch.bool, device=dev)                      # the elements that decay
    for name, off, k in opt.layout():
        sel[off:off + k] = name not in one_d
    results = {}
    for key, make in (("decoupled", lambda: opt), ("zero", lambda: FusedAdam(net.flat(), lr=1e-3, weight_decay=0.0))):
        flat.flat_p.copy_(start)
        o = make()
        for t in range(steps):
            _fill(flat, 200 + t)
            o.step()
        torch.cuda.synchronize()
        results[key] = flat.flat_p.clone()
    gs = [0.1 * torch.randn(flat.flat_g.numel(), generator=torch.Generator().manual_seed(200 + t)) for t in range(steps)]
    plain = _worst_ulp(results["zero"], _adam64(start, gs, sel, 1e-3, 0.0))
    decoupled = _worst_ulp(results["decoupled"], _adam64(start, gs, sel, 1e-3, 1e-2))
    print("UpperNet against float64, %d steps: plain step %.4f ulp_fp32(|p|), decoupled no_decay=1d %.4f" % (steps, plain, decoupled))
    _figures["fused_adam"] = (plain, decoupled)
    assert decoupled <= plain + steps
    assert _same_bits(results["decoupled"][~sel], results["zero"][~sel])                       # the 1-D tensors: a run at weight_decay 0
    assert not _same_bits(results["decoupled"][sel], results["zero"][sel])
    # the state round-trips, and a FRESH default optimiser takes the saved setting
    sd = opt.state_dict()
    assert sd["decoupled"] is True and sd["no_decay"] == sorted(one_d)
    twin = FusedAdam(net.flat(), lr=5.0)
    twin.load_state_dict(sd)
    assert twin.decoupled and twin.no_decay == opt.no_decay and _same_bits(twin._mask, opt._mask) and twin.weight_decay == 1e-2
    for o in (opt, twin):
        flat.flat_p.copy_(results["decoupled"])
        o.m.copy_(sd["m"]), o.v.copy_(sd["v"]), o.state.copy_(sd["state"])
        _fill(flat, 300)
        o.step()
        torch.cuda.synchronize()
        results[id(o)] = flat.flat_p.clone()
    assert _same_bits(results[id(opt)], results[id(twin)])
    # a mismatching optimiser refuses, and the message shows both
    for other in (FusedAdam(net.flat(), decoupled=True), FusedAdam(net.flat(), no_decay="1d"), FusedAdam(net.flat(), decoupled=True, no_decay=sorted(one_d)[:1])):
        with pytest.raises(ValueError) as e:
            other.load_state_dict(sd)
        assert "adamw (decoupled), no decay for %d tensors" % len(one_d) in str(e.value) and "this optimiser was built with" in str(e.value)
    with pytest.raises(ValueError, match="saved under the weight decay"):
        opt.load_state_dict(FusedAdam(net.flat(), **kw).state_dict())                           # (a state without the keys is coupled, all-decay)
    flat.flat_p.copy_(start)


# ---- 11. the step engines --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["upper", "imu", "finetune_all"])
def test_steps_hand_the_options_to_every_optimiser(dev, kind):
    import step_helpers
    from mmego_amd import nets
    from mmego_amd.train_step import ImuStep, StageStep

    def make(**kw):
        x, imu_in, body, target, R = step_helpers.batch(dev)
        torch.manual_seed(41)
        if kind == "imu":
            st = ImuStep(nets.IMUNet(15, 9, 64, 2, True, 0).to(dev).train(), lr=3e-5, use_graph=False, **kw)
            st.bind(imu_in, R, target)
            return st, [st.net]
        if kind == "upper":
            st = StageStep("upper", nets.UpperNet().to(dev).train(), None, lr=3e-5, weight_decay=1e-2, use_graph=False, **kw)
            st.bind(x, imu_in, body, target, R_gt=R)
            return st, [st.net]
        up, lo = nets.UpperNet().to(dev).train(), nets.LowerNet(64).to(dev).train()
        imu = nets.IMUNet(15, 9, 64, 2, True, 0).to(dev).train()
        st = StageStep("lower", lo, imu, upper_frozen=up, lr=3e-5, weight_decay=1e-2, imu_weight_decay=1e-2, use_graph=False, finetune_upper=True,
                       upper_lr=1e-5, finetune_imu=True, imu_lr=2e-5, **kw)
        st.bind(x, imu_in, body, target, R_gt=None)
        return st, [lo, up, imu]

    st, nets_ = make(decoupled=True, no_decay="1d")
    opts = st.optimisers()
    assert len(opts) == (3 if kind == "finetune_all" else 1)
    for opt in opts:
        one_d = sorted(k for k, p in opt.flat.module.named_parameters() if p.dim() <= 1)
        assert opt.decoupled and list(opt.no_decay) == one_d and opt.weight_decay == (1e-3 if kind == "imu" else 1e-2)
    assert _entry_points(lambda: [opt.step() for opt in opts]) == ["adam_step_decay"] * len(opts)
    for _ in range(2):
        st.step()
    torch.cuda.synchronize()
    assert all(opt.state[0].item() == 2 and bool(torch.isfinite(opt.flat.flat_p).all()) for opt in opts)
    # with the options off the step is today's, bit for bit: the same launches and the same fingerprint as a step built without them
    prints = []
    for kw in (dict(), dict(decoupled=False, no_decay=None)):
        st, nets_ = make(**kw)
        assert all(not opt.decoupled and opt.no_decay == () and opt._mask is None for opt in st.optimisers())
        assert set(_entry_points(lambda: [opt.step() for opt in st.optimisers()])) == {"adam_step"}
        for _ in range(2):
            st.step()
        torch.cuda.synchronize()
        prints.append([(k, step_helpers.sha256(t)) for k, t in step_helpers.state(st, nets_)])
    assert prints[0] == prints[1]


# ---- 12. the command line --------------------------------------------------------------------------------------------------------------------------
def _ckpt(out_dir, idx, epoch):
    f = [f for f in glob.glob(os.path.join(out_dir, "model", str(idx), "epoch%d_*.pth" % epoch)) if not f.endswith(".train_state.pth")]
    assert len(f) == 1, f
    return f[0]


def test_cli_upper_net_two_epochs_equal_one_plus_resume(tmp_path):
    """--train --network Upper_Net --weight_decay 0.01 --decay_mode adamw --no_decay_1d --lr_schedule cosine --lr_warmup 2: two epochs in one
    go against one epoch and --resume WITHOUT the decay flags (the optimiser state carries them), on the synthetic Sample_data tree of
    tests/test_cli_gpu.py, as test_lr_schedule_gpu's test of this name (the command line reads a tree of .mat frames, which the committed
    real windows are not)."""
    from test_cli_gpu import _make_dataset, _run
    data = str(tmp_path / "Sample_data")
    _make_dataset(data, np.random.default_rng(1))
    out_dir = str(tmp_path / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    base = ["--train", "--network", "Upper_Net", "--gt_head_pose", "--data_root", data, "--batch_size", "1", "--device", "cuda:0", "--seed", "5"]
    sched = ["--lr_schedule", "cosine", "--lr_warmup", "2", "--lr_decay_steps", "8"]
    flags = ["--weight_decay", "0.01", "--decay_mode", "adamw", "--no_decay_1d"]
    line = "[mmego_amd] weight decay (Upper_Net): adamw, W 0.01; "
    out = _run(base + sched + flags + ["--epochs", "2", "--log_dir", "9191"], env)
    assert out.count(line) == 1 and "tensors and" in out
    out = _run(base + sched + flags + ["--epochs", "1", "--log_dir", "9192"], env)
    first = _ckpt(out_dir, 9192, 0)
    out = _run(base + ["--epochs", "2", "--log_dir", "9193", "--resume", first], env)
    assert "resumed from" in out and "epoch: 2" in out and out.count(line) == 1
    a, b = _ckpt(out_dir, 9191, 1), _ckpt(out_dir, 9193, 1)
    sa, sb = torch.load(a, map_location="cpu"), torch.load(b, map_location="cpu")
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    ta = torch.load(a[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)["optimizer"]
    tb = torch.load(b[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)["optimizer"]
    for k in ("m", "v", "state"):
        assert torch.equal(ta[k], tb[k]), k
    assert ta["decoupled"] is tb["decoupled"] is True and ta["no_decay"] == tb["no_decay"] and len(ta["no_decay"]) > 0
    assert ta["weight_decay"] == tb["weight_decay"] == 0.01 and ta["state"][0].item() == 8
    # a resume that names another decay ends with the message, before any epoch
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + base + ["--epochs", "2", "--log_dir", "9194", "--resume", first,
                                                                               "--weight_decay", "0.01"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--resume: the training state was saved under the weight decay" in r.stderr, r.stderr[-2000:]
    assert "epoch: 2" not in r.stdout
