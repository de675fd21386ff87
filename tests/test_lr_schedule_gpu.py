"""GPU: the fused Adam steps with a learning-rate schedule evaluated inside the launch (csrc/optim.hip: mmego_adam_step_sched),
FusedAdam's lr_schedule / current_lr(), the step engines' lr_schedule and `main.py --train --lr_schedule`.

Sizes as tests/test_ema_gpu.py: 4 floats (one lane), 1028 (a partial workgroup), 2 097 156 (exactly one lane takes a second grid-stride
trip).  Schedules short enough that 7 steps cross every regime: W = 3, D = 3, and for the step kind E = 2, g = 0.5, r = 0.2 -- t = 1 and 2
warm up, t = 3 = W is the first step at the full rate, t = 4, 5, 6 = W + D decay, t = 7 holds.

state[3] against float64 (tests/lr_schedule_ref.py): lr_t = lr * (w * d) is about a dozen double roundings of quantities <= 1, cos and pow
within a few ulp and the argument error of pi * x: under 2e-15 * lr on each side.  The bound is 1e-14 * lr."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from adam_helpers import ADAM, LR, AdamSet as _Set, grads as _seeded, same_bits as _same_bits
from conftest import ROOT
from lr_schedule_ref import mult_ref
from step_helpers import entry_points as _entry_points

pytestmark = pytest.mark.gpu

SIZES = [4, 1028, 2048 * 256 * 4 + 4]
SENTINEL = -7.5
BOUND = 1e-14
STEPS = 7
# kind -> (the MmegoLrSchedule fields, the reference's arguments)
KINDS = {
    "constant": (dict(kind=0, warmup=3.0), dict(W=3)),
    "cosine": (dict(kind=1, warmup=3.0, span=3.0, floor=0.1), dict(W=3, D=3, r=0.1)),
    "linear": (dict(kind=2, warmup=3.0, span=3.0, floor=0.1), dict(W=3, D=3, r=0.1)),
    "step": (dict(kind=3, warmup=3.0, floor=0.2, every=2.0, gamma=0.5), dict(W=3, r=0.2, E=2, g=0.5)),
}
FORMS = [(None, None), (0.9, None), (None, "half"), (0.9, "half")]          # (ema decay, max_norm): plain, averaged, clipped, both
_worst = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _sched(kind):
    from mmego_amd import hip
    return hip.LrSchedule(**KINDS[kind][0])


def _ref(kind, t):
    return mult_ref(kind, t, **KINDS[kind][1])


def _grads(dev, n):
    """(p0, [g_1 .. g_7]) on the device."""
    return _seeded(dev, n, STEPS)


def _max_norm(form, grads):
    """Half the first gradient's norm: clipping is live."""
    return None if form is None else 0.5 * float(grads[0].double().pow(2).sum().sqrt())


# ---- 1. the scheduled step is the existing step at lr_t ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("n", SIZES)
def test_scheduled_step_is_the_existing_step_at_its_rate(dev, n, wd, kind):
    p0, grads = _grads(dev, n)
    sched = _sched(kind)
    for decay, clip in FORMS:
        c = _max_norm(clip, grads)
        a, b = _Set(dev, p0, 4), _Set(dev, p0, 3)
        rates = []
        for t, g in enumerate(grads, 1):
            a.sched_step(g, wd, sched, decay=decay, max_norm=c)
            rate = a.state[3].item()
            rates.append(rate)
            b.step(g, wd, decay=decay, max_norm=c, lr=rate)
            assert a.same(b), (decay, clip, t)
            assert a.state[0].item() == t and a.ticket.item() == 0
        assert rates[2] == LR and rates[0] < rates[1] < rates[2]
        assert rates[6] == rates[5] or kind == "step"                       # (past the span; the step kind has none: it reaches r at t = 9)
        if c is not None:
            assert a.stats[4].item() >= 1 and a.stats[3].item() == STEPS
        if decay is None:
            assert _same_bits(a.ema, p0)                                    # (no average asked for: none touched)
        else:
            assert not _same_bits(a.ema, p0)
        assert not _same_bits(a.p, p0)


# ---- 2. state[3] against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_rate_against_float64(dev, kind):
    sched = _sched(kind)
    worst = 0.0
    for n in SIZES[:2]:
        p0, grads = _grads(dev, n)
        for decay, clip in FORMS:
            a = _Set(dev, p0, 4)
            rates = []
            # (the step kind reaches its lower bound at t = 9, s = 6: g^3 = 0.125 < r; it gets three more steps, on gradients used before)
            for t, g in enumerate(grads + (grads[:3] if kind == "step" else []), 1):
                a.sched_step(g, 1e-3, sched, decay=decay, max_norm=_max_norm(clip, grads))
                rate = a.state[3].item()
                rates.append(rate)
                err = abs(rate - LR * _ref(kind, t))
                worst = max(worst, err / (BOUND * LR))
                assert err <= BOUND * LR, (kind, n, t, rate, LR * _ref(kind, t))
            assert rates[2] == LR                                           # s == 0 and t >= W: exactly lr
            if kind == "step":
                assert rates[3] == LR                                       # (t = 4: g^floor(1 / 2) = g^0, exactly 1)
            assert abs(rates[0] - LR * (1.0 / 3.0)) <= BOUND * LR
            if kind == "step":
                assert rates[6] < rates[5] and rates[8] == rates[9] == LR * 0.2 and rates[7] == rates[6]
            else:
                assert rates[6] == rates[5]                                 # it holds past the span
            if kind == "constant":
                assert rates[3:] == [LR] * 4
            else:
                assert rates[3] >= rates[4] >= rates[5] and rates[5] < LR
    print("%s: worst |state[3] - lr * float64 multiplier| / (1e-14 * lr) = %.4f" % (kind, worst))
    _worst[kind] = worst


# ---- 3. a constant schedule without warm-up is the plain step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_constant_schedule_without_warm_up_is_the_unscheduled_step(dev, n):
    from mmego_amd import hip
    p0, grads = _grads(dev, n)
    sched = hip.LrSchedule(kind=0)
    for decay, clip in FORMS:
        c = _max_norm(clip, grads)
        a, b = _Set(dev, p0, 4), _Set(dev, p0, 3)
        for t, g in enumerate(grads[:3], 1):
            a.sched_step(g, 1e-3, sched, decay=decay, max_norm=c)
            b.step(g, 1e-3, decay=decay, max_norm=c)
            assert a.same(b), (decay, clip, t)
            assert a.state[3].item() == LR


# ---- 4. a non-finite gradient does not consume a schedule step ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cosine", "step"])
@pytest.mark.parametrize("n", SIZES)
def test_non_finite_gradient_consumes_no_schedule_step(dev, n, kind):
    p0, grads = _grads(dev, n)
    sched = _sched(kind)
    a = _Set(dev, p0, 4)
    a.sched_step(grads[0], 1e-3, sched, decay=0.9, max_norm=1.0)
    keep = a.snapshot(stats=True, ema=True)
    g = grads[1].clone()
    g[n - 3] = float("inf")
    a.sched_step(g, 1e-3, sched, decay=0.9, max_norm=1.0)
    after = a.snapshot(stats=True, ema=True)
    for i, (x, y) in enumerate(zip(after, keep)):
        if i != 4:                                                          # (everything but the statistics, all four state words included)
            assert _same_bits(x, y), i
    assert a.stats[5].item() == 1 and a.stats[3].item() == 2 and a.ticket.item() == 0 and a.state[0].item() == 1
    a.sched_step(grads[1], 1e-3, sched, decay=0.9, max_norm=1.0)
    torch.cuda.synchronize()
    assert a.state[0].item() == 2 and abs(a.state[3].item() - LR * _ref(kind, 2)) <= BOUND * LR
    b = _Set(dev, p0, 4)                                                    # (the two finite steps without the bad one in between)
    for g in grads[:2]:
        b.sched_step(g, 1e-3, sched, decay=0.9, max_norm=1.0)
    for x, y in zip(a.tensors()[:4], b.tensors()[:4]):
        assert _same_bits(x, y)
    assert _same_bits(a.state, b.state)


# ---- 5. capture --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cosine", "linear"])
@pytest.mark.parametrize("clip", [None, "half"])
def test_one_captured_launch_replays_another_rate_every_step(dev, clip, kind):
    from mmego_amd import ops
    n = SIZES[1]
    p0, grads = _grads(dev, n)
    sched = _sched(kind)
    c = _max_norm(clip, grads)
    a, b = _Set(dev, p0, 4), _Set(dev, p0, 4)
    for g in grads:
        a.sched_step(g, 1e-3, sched, decay=0.9, max_norm=c)
    torch.cuda.synchronize()
    gbuf = torch.zeros(n, device=dev)
    graph = torch.cuda.CUDAGraph()
    with ops.capture(graph):
        b.sched_step(gbuf, 1e-3, sched, decay=0.9, max_norm=c)
    torch.cuda.synchronize()
    assert not bool(b.state.any()) and _same_bits(b.p, p0) and _same_bits(b.ema, p0)         # (capturing executes nothing)
    rates = set()
    for g in grads:
        gbuf.copy_(g)
        graph.replay()
        rates.add(b.state[3].item())
    assert a.same(b) and _same_bits(a.state, b.state) and b.state[0].item() == STEPS
    assert len(rates) >= 5, sorted(rates)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    from mmego_amd import hip
    n = 1028
    nb = hip.lib().mmego_grad_norm_nblk(n)
    buf = {k: torch.full((n + 8,), SENTINEL, device=dev) for k in "pgmve"}
    part = torch.full((nb + 1,), SENTINEL, dtype=torch.float64, device=dev)
    state8 = torch.zeros(8, dtype=torch.float64, device=dev)
    state = state8[:4]
    stats = torch.zeros(8, dtype=torch.float64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    nan, inf = float("nan"), float("inf")
    good = dict(p=buf["p"], g=buf["g"], m=buf["m"], v=buf["v"], n=n, state=state, lr=LR, skip=None, nskip=0, ticket=ticket, part=part,
                npart=nb, max_norm=1.0, stats=stats, ema=buf["e"], ema_decay=0.9, sched=_sched("cosine"))
    plain = dict(part=None, npart=0, max_norm=0.0, stats=None)
    no_avg = dict(ema=None, ema_decay=0.0)

    def call(**kw):
        a = dict(good, **kw)
        hip.call("adam_step_sched", a["p"], a["g"], a["m"], a["v"], a["n"], a["state"], a["lr"], *ADAM[1:], 1e-3, a["skip"], a["nskip"],
                 a["ticket"], a["part"], a["npart"], a["max_norm"], a["stats"], a["ema"], a["ema_decay"], a["sched"])

    def sched(base="cosine", **kw):
        return hip.LrSchedule(**dict(KINDS[base][0], **kw))

    misaligned_state = torch.zeros(9, dtype=torch.float32, device=dev)[1:].view(torch.uint8)       # (4 bytes off an 8-byte boundary)
    bad = [
        # what the existing entry points refuse
        dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(state=None), dict(ticket=None), dict(n=0), dict(n=1026),
        dict(p=buf["p"][1:]), dict(g=buf["g"][1:]), dict(m=buf["m"][2:]), dict(v=buf["v"][3:]),
        dict(skip=torch.tensor([2, 8], dtype=torch.int64), nskip=1), dict(skip=torch.tensor([8, 4], dtype=torch.int64), nskip=1),
        dict(skip=None, nskip=1), dict(nskip=5, skip=torch.zeros(10, dtype=torch.int64)), dict(skip=torch.tensor([0, n + 4], dtype=torch.int64), nskip=1),
        dict(npart=nb + 1), dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=nan), dict(part=part[1:].view(torch.float32)[1:]),
        dict(stats=stats.view(torch.float32)[1:]),
        dict(ema=buf["e"][1:]), dict(ema_decay=0.0), dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=nan), dict(ema_decay=1.5),
        # the schedule
        dict(sched=None), dict(sched=sched(kind=4)), dict(sched=sched(kind=-1)), dict(sched=sched(reserved=1)),
        dict(sched=sched(warmup=-1.0)), dict(sched=sched(warmup=2.5)), dict(sched=sched(warmup=nan)), dict(sched=sched(warmup=inf)),
        dict(sched=sched(span=0.0)), dict(sched=sched(span=0.5)), dict(sched=sched(span=2.5)), dict(sched=sched(span=nan)), dict(sched=sched(span=inf)),
        dict(sched=sched("linear", span=0.0)), dict(sched=sched("linear", span=1.5)), dict(sched=sched("linear", span=nan)),
        dict(sched=sched("linear", span=-inf)),
        dict(sched=sched(floor=1.0)), dict(sched=sched(floor=-0.1)), dict(sched=sched(floor=nan)), dict(sched=sched("constant", floor=1.5)),
        dict(sched=sched("step", floor=1.0)),
        dict(sched=sched("step", every=0.0)), dict(sched=sched("step", every=1.5)), dict(sched=sched("step", every=nan)),
        dict(sched=sched("step", every=inf)), dict(sched=sched("step", gamma=0.0)), dict(sched=sched("step", gamma=-0.5)),
        dict(sched=sched("step", gamma=1.5)), dict(sched=sched("step", gamma=nan)),
        # state, and the arguments that come in groups
        dict(state=misaligned_state),
        dict(part=None), dict(stats=None), dict(part=None, npart=0), dict(part=None, stats=None), dict(part=None, npart=0, stats=stats),
        dict(plain, npart=nb), dict(plain, stats=stats),
        dict(ema=None), dict(plain, ema=None, ema_decay=0.9),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError, match="bad argument"):
            call(**kw)
        if "sched" in kw or "state" in kw:                                 # (the plain form and the form without an average refuse alike)
            with pytest.raises(RuntimeError, match="bad argument"):
                call(**dict(plain, **dict(no_avg, **kw)))
    s = sched(kind=7)
    rc = hip.lib().mmego_adam_step_sched(hip.stream_handle(), buf["p"].data_ptr(), buf["g"].data_ptr(), buf["m"].data_ptr(), buf["v"].data_ptr(), n,
                                         state.data_ptr(), *ADAM, 1e-3, None, 0, ticket.data_ptr(), None, 0, 0.0, None, None, 0.0,
                                         __import__("ctypes").addressof(s))
    assert rc != 0                                                           # (the return code itself)
    torch.cuda.synchronize()
    for t in list(buf.values()) + [part]:
        assert bool((t == SENTINEL).all())
    assert not bool(state8.any()) and not bool(stats.any()) and ticket.item() == 0 and not bool(misaligned_state.any())
    # and what is not refused: the fields a kind does not read may hold anything
    live = {k: torch.zeros(n, device=dev) for k in "pgmv"}
    hip.call("adam_step_sched", live["p"], live["g"], live["m"], live["v"], n, state, *ADAM, 0.0, None, 0, ticket, None, 0, 0.0, None, None, 0.0,
             hip.LrSchedule(kind=0, span=nan, every=-1.0, gamma=nan))
    torch.cuda.synchronize()
    assert state[0].item() == 1 and state[3].item() == LR and ticket.item() == 0


# ---- 7. FusedAdam ------------------------------------------------------------------------------------------------------------------------------
def _tiny_imu(dev):
    from mmego_amd import nets
    torch.manual_seed(7)
    return nets.IMUNet(15, 9, 32, 2, True, 0).to(dev).train()


def _fill_grad(flat, dead, seed):
    flat.flat_g.copy_(torch.randn(flat.flat_g.numel(), generator=torch.Generator().manual_seed(seed)))
    flat.flat_g[dead] = float("nan")                                        # (grad=None for torch: read neither into the update nor the norm)


def test_fused_adam_with_a_schedule(dev):
    """On a tiny IMUNet (fc3 never trains: a skip range), as tests/test_clip_grad_norm_gpu.py builds it."""
    from mmego_amd.params import FusedAdam, LrSchedule
    from mmego_amd.train_step import empty_step
    sched = LrSchedule("cosine", warmup=3, span=3, floor=0.1)
    net = _tiny_imu(dev)
    flat = net.flat().ensure()
    kw = dict(lr=1e-3, weight_decay=1e-3)
    # without a schedule: the names recorded today, three state words, the state_dict keys of today
    assert _entry_points(FusedAdam(net.flat(), **kw).step) == ["adam_step"]
    assert _entry_points(FusedAdam(net.flat(), max_grad_norm=0.5, **kw).step) == ["grad_sqnorm", "adam_step_clipped"]
    assert _entry_points(FusedAdam(net.flat(), ema_decay=0.9, **kw).step) == ["adam_step_ema"]
    assert _entry_points(FusedAdam(net.flat(), max_grad_norm=0.5, ema_decay=0.9, **kw).step) == ["grad_sqnorm", "adam_step_clipped_ema"]
    off = FusedAdam(net.flat(), **kw)
    off._ensure()
    assert off.state.numel() == 3 and "lr_schedule" not in off.state_dict() and off.current_lr() == 1e-3
    # with one: the one entry point, the norm pass ahead of it when clipping
    for extra in (dict(), dict(ema_decay=0.9)):
        assert _entry_points(FusedAdam(net.flat(), lr_schedule=sched, **kw, **extra).step) == ["adam_step_sched"]
        assert _entry_points(FusedAdam(net.flat(), lr_schedule=sched, max_grad_norm=0.5, **kw, **extra).step) == ["grad_sqnorm", "adam_step_sched"]
    opt = FusedAdam(net.flat(), lr_schedule=sched, max_grad_norm=0.5, ema_decay=0.9, **kw)
    assert _entry_points(lambda: empty_step(net, opt, None))[-1] == "adam_step_sched"      # (a rank with an empty shard: the same launch)
    dead = torch.zeros(flat.flat_p.numel(), dtype=torch.bool, device=dev)
    for prm, o in zip(flat.params, flat.offsets):
        if any(prm is q for q in net.never_trained()):
            dead[o:o + (prm.numel() + 3) // 4 * 4] = True
    assert bool(dead.any()) and not bool(dead.all())
    start = flat.flat_p.clone()
    assert opt.current_lr() == 1e-3 * _ref("cosine", 1) and opt.state.numel() == 4           # (before the first step: from the host)
    # 7 steps uninterrupted; a second optimiser takes 3, is saved, and a FRESH one continues from its state_dict
    for t in range(1, STEPS + 1):
        _fill_grad(flat, dead, 100 + t)
        opt.step()
        assert abs(opt.current_lr() - 1e-3 * _ref("cosine", t)) <= BOUND * 1e-3, t
    torch.cuda.synchronize()
    want = [flat.flat_p.clone(), opt.m.clone(), opt.v.clone(), opt.state.clone(), opt.ema.clone()]
    assert _same_bits(flat.flat_p[dead], start[dead]) and _same_bits(opt.ema[dead], start[dead])    # the skip range is left alone
    assert bool(torch.isfinite(flat.flat_p).all()) and opt.state[0].item() == STEPS
    flat.flat_p.copy_(start)
    first = FusedAdam(net.flat(), lr_schedule=sched, max_grad_norm=0.5, ema_decay=0.9, **kw)
    for t in range(1, 4):
        _fill_grad(flat, dead, 100 + t)
        first.step()
    sd = first.state_dict()
    assert sd["lr_schedule"] == sched.to_dict() and sd["state"].numel() == 4 and sd["state"][3].item() == 1e-3
    second = FusedAdam(net.flat(), lr=5.0, lr_schedule=LrSchedule.from_dict(sd["lr_schedule"]), max_grad_norm=0.5, ema_decay=0.9)
    second.load_state_dict(sd)
    assert second.current_lr() == 1e-3
    for t in range(4, STEPS + 1):
        _fill_grad(flat, dead, 100 + t)
        second.step()
    torch.cuda.synchronize()
    for x, y in zip(want, [flat.flat_p, second.m, second.v, second.state, second.ema]):
        assert _same_bits(x, y)
    # a differing saved schedule is refused, and the message names both
    other = LrSchedule("linear", warmup=3, span=3, floor=0.1)
    for dst in (FusedAdam(net.flat(), lr_schedule=other), FusedAdam(net.flat())):
        with pytest.raises(ValueError) as e:
            dst.load_state_dict(sd)
        assert repr(sched) in str(e.value) and repr(dst.lr_schedule) in str(e.value)


# ---- 8. the step engines -----------------------------------------------------------------------------------------------------------------------
RATES = {"opt": 3e-5, "upper_opt": 1e-5, "imu_opt": 2e-5}


def _make_step(dev, kind, use_graph, sched):
    import step_helpers
    from mmego_amd import nets
    from mmego_amd.train_step import ImuStep, StageStep
    x, imu_in, body, target, R = step_helpers.batch(dev)
    torch.manual_seed(41)
    if kind == "imu":
        st = ImuStep(nets.IMUNet(15, 9, 64, 2, True, 0).to(dev).train(), lr=RATES["opt"], use_graph=use_graph, lr_schedule=sched)
        st.bind(imu_in, R, target)
    elif kind == "upper":
        st = StageStep("upper", nets.UpperNet().to(dev).train(), None, lr=RATES["opt"], use_graph=use_graph, lr_schedule=sched)
        st.bind(x, imu_in, body, target, R_gt=R)
    else:                                                                   # (the step of --finetune_all: three nets, three rates)
        up, lo = nets.UpperNet().to(dev).train(), nets.LowerNet(64).to(dev).train()
        imu = nets.IMUNet(15, 9, 64, 2, True, 0).to(dev).train()
        st = StageStep("lower", lo, imu, upper_frozen=up, lr=RATES["opt"], use_graph=use_graph, finetune_upper=True, upper_lr=RATES["upper_opt"],
                       finetune_imu=True, imu_lr=RATES["imu_opt"], lr_schedule=sched)
        st.bind(x, imu_in, body, target, R_gt=None)
    return st


@pytest.mark.parametrize("kind", ["upper", "imu", "finetune_all"])
def test_steps_hand_one_schedule_to_every_optimiser(dev, kind):
    import step_helpers
    from mmego_amd.params import LrSchedule
    sched = LrSchedule("cosine", warmup=3, span=3, floor=0.1)
    k = 5
    runs = []
    for use_graph in (True, False):
        st = _make_step(dev, kind, use_graph, sched)
        keys = [o for o, _ in step_helpers.TRAINED if getattr(st, o, None) is not None]
        assert keys == (["opt", "imu_opt", "upper_opt"] if kind == "finetune_all" else ["opt"])
        assert all(getattr(st, o).lr_schedule is sched and getattr(st, o).lr == RATES[o] for o in keys)
        launched = _entry_points(lambda: [opt.step() for opt in st.optimisers()])
        assert launched == ["adam_step_sched"] * len(keys)
        for _ in range(k):
            st.step()
        torch.cuda.synchronize()
        for o in keys:
            opt = getattr(st, o)
            assert opt.state[0].item() == k
            err = abs(opt.state[3].item() - RATES[o] * _ref("cosine", k))
            print("%s graph=%s %s: |state[3] - lr * float64 multiplier| / (1e-14 * lr) = %.4f" % (kind, use_graph, o, err / (BOUND * RATES[o])))
            assert err <= BOUND * RATES[o], (kind, use_graph, o)
            assert opt.current_lr() == opt.state[3].item()
        runs.append([t.clone() for o in keys for t in (getattr(st, o).flat.flat_p, getattr(st, o).m, getattr(st, o).v, getattr(st, o).state)])
    for x, y in zip(*runs):                                                # graph and eager: the same bits in weights and state
        assert _same_bits(x, y)
    # without the option the optimisers are the ones of today
    st = _make_step(dev, kind, False, None)
    assert all(opt.lr_schedule is None for opt in st.optimisers())
    assert set(_entry_points(lambda: [opt.step() for opt in st.optimisers()])) == {"adam_step"}


@pytest.mark.parametrize("kind", ["concurrent", "shared", "pipelined"])
def test_engines_around_scheduled_stages_run_unchanged(dev, kind):
    """ConcurrentStages, SharedImuStages and PipelinedStages around an Upper and a Lower StageStep that carry a schedule (the arrangement of
    step_helpers._two_stage): every stage's optimiser takes the scheduled launch at its own count."""
    import step_helpers
    from mmego_amd import nets
    from mmego_amd.params import LrSchedule
    from mmego_amd.train_step import ConcurrentStages, PipelinedStages, SharedImuStages, StageStep
    sched = LrSchedule("linear", warmup=3, span=3, floor=0.1)
    x, imu_in, body, target, R = step_helpers.batch(dev)
    torch.manual_seed(43)
    imu_u, imu_l = nets.IMUNet(15, 9, 64, 2).to(dev).eval(), nets.IMUNet(15, 9, 64, 2).to(dev).eval()
    up, lo, fr = nets.UpperNet().to(dev).train(), nets.LowerNet(64).to(dev).train(), nets.UpperNet().to(dev).eval()
    own = kind == "concurrent"
    su = StageStep("upper", up, imu_u if own else None, lr=3e-5, use_graph=False, lr_schedule=sched)
    sl = StageStep("lower", lo, imu_l if own else None, upper_frozen=fr, lr=1e-5, use_graph=False, lr_schedule=sched)
    if kind == "concurrent":
        eng = ConcurrentStages([su, sl], use_graph=True)
    elif kind == "shared":
        eng = SharedImuStages(imu_u, [su, sl], imu_in, use_graph=True)
    else:
        eng = PipelinedStages([su, sl], [imu_u, imu_l], imu_in, use_graph=True)
    for st in (su, sl):
        st.bind(x, imu_in, body, target)
    if kind == "pipelined":
        eng.prime()
    k = 5
    for _ in range(k):
        eng.step()
    torch.cuda.synchronize()
    for st, lr in ((su, 3e-5), (sl, 1e-5)):
        assert st.opt.state.tolist()[0] == k and abs(st.opt.current_lr() - lr * _ref("linear", k)) <= BOUND * lr
        assert bool(torch.isfinite(st.opt.flat.flat_p).all())


# ---- 9. the command line -----------------------------------------------------------------------------------------------------------------------
DECAY_STEPS = 8
START = "[mmego_amd] learning-rate schedule: cosine, warm-up 2 steps, span %d steps, floor 0.1" % DECAY_STEPS


def _ckpt(out_dir, idx, epoch):
    f = [f for f in glob.glob(os.path.join(out_dir, "model", str(idx), "epoch%d_*.pth" % epoch)) if not f.endswith(".train_state.pth")]
    assert len(f) == 1, f
    return f[0]


def _lr_lines(out):
    return [float(ln.split(":")[1]) for ln in out.splitlines() if ln.startswith("LR (Upper_Net):")]


def test_cli_upper_net_two_epochs_equal_one_plus_resume(tmp_path):
    """--train --network Upper_Net --lr_schedule cosine --lr_warmup 2 --lr_decay_steps 8 --lr_min_ratio 0.1: two epochs in one go against
    one epoch and --resume WITHOUT the flags (the optimiser state carries the schedule).  The synthetic tree has four training windows: at
    --batch_size 1 an epoch is four optimiser steps, so epoch 1 ends at t = 4 (two steps into the decay) and epoch 2 at t = 8 (six)."""
    from test_cli_gpu import _make_dataset, _run
    data = str(tmp_path / "Sample_data")
    _make_dataset(data, np.random.default_rng(1))
    out_dir = str(tmp_path / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    base = ["--train", "--network", "Upper_Net", "--gt_head_pose", "--data_root", data, "--batch_size", "1", "--device", "cuda:0", "--seed", "5"]
    flags = ["--lr_schedule", "cosine", "--lr_warmup", "2", "--lr_decay_steps", str(DECAY_STEPS), "--lr_min_ratio", "0.1"]
    out = _run(base + flags + ["--epochs", "2", "--log_dir", "9181"], env)
    assert out.count(START) == 1
    lrs = _lr_lines(out)
    assert len(lrs) == 2 and lrs[1] < lrs[0], lrs                            # one line per epoch, and the values fall
    log = open(os.path.join(out_dir, "report", "9181", "log-eval.txt")).read()
    assert log.count("LR (Upper_Net):") == 2
    out = _run(base + flags + ["--epochs", "1", "--log_dir", "9182"], env)
    assert out.count(START) == 1 and _lr_lines(out) == lrs[:1]
    first = _ckpt(out_dir, 9182, 0)
    out = _run(base + ["--epochs", "2", "--log_dir", "9183", "--resume", first], env)
    assert "resumed from" in out and "epoch: 2" in out and "epoch: 1\n" not in out and out.count(START) == 1
    assert _lr_lines(out) == lrs[1:]
    a, b = _ckpt(out_dir, 9181, 1), _ckpt(out_dir, 9183, 1)
    sa, sb = torch.load(a, map_location="cpu"), torch.load(b, map_location="cpu")
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    ta = torch.load(a[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)["optimizer"]
    tb = torch.load(b[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)["optimizer"]
    for k in ("m", "v", "state"):
        assert torch.equal(ta[k], tb[k]), k
    want = dict(kind="cosine", warmup=2, span=DECAY_STEPS, floor=0.1, every=None, gamma=None)
    assert ta["lr_schedule"] == tb["lr_schedule"] == want and ta["state"].numel() == 4
    t, lr = ta["state"][0].item(), ta["lr"]
    assert t == 8 and abs(ta["state"][3].item() - lr * mult_ref("cosine", t, W=2, D=DECAY_STEPS, r=0.1)) <= BOUND * lr
    assert abs(lrs[1] - ta["state"][3].item()) <= 1e-8 * lr                  # (the line prints nine digits)
    # a resume that names another schedule ends with the message, before any epoch
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + base + ["--epochs", "2", "--log_dir", "9184", "--resume", first,
                                                                               "--lr_schedule", "linear", "--lr_decay_steps", str(DECAY_STEPS)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--resume: the training state was saved under the learning-rate schedule" in r.stderr, r.stderr[-2000:]
    assert "epoch: 2" not in r.stdout
