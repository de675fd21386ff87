"""GPU: the fused Adam steps with a weight average (csrc/optim.hip: mmego_adam_step_ema, mmego_adam_step_clipped_ema), FusedAdam's
ema_decay / averaged() / ema_state_dict(), the step engines' ema_decay and `main.py --train --ema_decay`.

Sizes: 4 floats (one float4, one lane), 1028 (a partial workgroup), 2 097 156 = 524 289 float4: the launch is capped at 2048 workgroups
of 256 lanes = 524 288 lanes, so exactly one lane -- the first -- takes a second grid-stride trip, for the last float4.

The average against float64: e_k = e_{k-1} + (1 - d)(p_k - e_{k-1}) in double on the recorded fp32 p_k.  The kernel rounds twice per step
and element (the difference, the fma; omd = (float)(1 - d) adds a third, relative 2^-24 on a term of at most (1 - d) |p - e|), so after k
steps |ema - e_k| <= k * 2^-23 * max(|p_k|, |e_k|) per element."""
import glob
import os

import numpy as np
import pytest
import torch

from adam_helpers import ADAM, AdamSet as _Set, grads as _seeded, same_bits as _same_bits
from conftest import ROOT
from step_helpers import entry_points as _entry_points

pytestmark = pytest.mark.gpu

SIZES = [4, 1028, 2048 * 256 * 4 + 4]
SENTINEL = -7.5
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _grads(dev, n):
    """(p0, [g_1, g_2, g_3]) on the device."""
    return _seeded(dev, n, 3)


# ---- 1. the Adam part is the plain step, plain and clipped ----------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("n", SIZES)
def test_adam_part_is_the_plain_step(dev, n, wd):
    p0, grads = _grads(dev, n)
    plain, avg, clip, clip_avg, open_avg = (_Set(dev, p0) for _ in range(5))
    norm = float(grads[0].double().pow(2).sum().sqrt())
    c = 0.5 * norm                                                          # (half the first step's norm: that step is clipped)
    for k, g in enumerate(grads, 1):
        plain.step(g, wd)
        avg.step(g, wd, decay=0.9)
        clip.step(g, wd, max_norm=c)
        clip_avg.step(g, wd, decay=0.9, max_norm=c)
        open_avg.step(g, wd, decay=0.9, max_norm=float("inf"))
        assert avg.same_adam(plain), k
        assert clip_avg.same_adam(clip) and torch.equal(clip_avg.stats, clip.stats), k
        # max_norm = inf: the clip factor is exactly 1, so the clipped form is the plain form, average included
        assert open_avg.same_adam(plain) and _same_bits(open_avg.ema, avg.ema), k
        assert plain.state[0].item() == k and all(s.ticket.item() == 0 for s in (avg, clip_avg, open_avg))
    assert clip.stats[4].item() >= 1 and clip.stats[3].item() == 3
    assert not _same_bits(avg.ema, p0) and not _same_bits(avg.ema, avg.p)
    assert not bool(plain.ema.ne(p0).any())                                 # (the plain entry points know no average)


# ---- 2. the average against float64 -----------------------------------------------------------------------------------------------------------
def _check_recurrence(e0, snapshots, ema_after, decay, what):
    """ema_after[k-1] against the float64 recurrence on the recorded parameters; prints the worst error over the bound."""
    e = e0.double()
    for k, (p, got) in enumerate(zip(snapshots, ema_after), 1):
        e = e + (1.0 - decay) * (p.double() - e)
        bound = k * EPS * torch.maximum(p.double().abs(), e.abs())
        err = (got.double() - e).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("%s: decay %g, step %d: worst |ema - float64| / bound = %.3f" % (what, decay, k, worst))
        assert bool((err <= bound).all()), (what, decay, k, worst)


@pytest.mark.parametrize("decay", [0.9, 0.999])
@pytest.mark.parametrize("n", SIZES)
def test_average_against_float64(dev, n, decay):
    p0, grads = _grads(dev, n)
    for clipped in (False, True):
        a = _Set(dev, p0)
        ps, es = [], []
        for g in grads:
            a.step(g, 1e-3, decay=decay, max_norm=1.0 if clipped else None)
            torch.cuda.synchronize()
            ps.append(a.p.clone())
            es.append(a.ema.clone())
        _check_recurrence(p0, ps, es, decay, "n=%d %s" % (n, "clipped" if clipped else "plain"))


# ---- 3. skip ranges -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("n", SIZES[1:])
def test_skip_ranges_leave_the_average_alone(dev, n, clipped):
    """Two float4-aligned ranges; the second holds the buffer's last float4, which at the large size is the one the second trip takes."""
    p0, grads = _grads(dev, n)
    skip = torch.tensor([8, 24, n - 8, n], dtype=torch.int64)
    dead = torch.zeros(n, dtype=torch.bool, device=dev)
    dead[8:24] = True
    dead[n - 8:] = True
    a, b = _Set(dev, p0), _Set(dev, p0)
    a.ema.copy_(p0 * 0.5 + 10.0)                                            # (an average far from the weights everywhere: every live one moves)
    b.ema.copy_(a.ema)
    e0 = a.ema.clone()
    for g in grads:
        g = g.clone()
        g[dead] = float("nan")                                              # (grad=None for torch: neither read into the update nor the norm)
        a.step(g, 1e-3, decay=0.9, max_norm=1.0 if clipped else None, skip=skip)
        b.step(g, 1e-3, max_norm=1.0 if clipped else None, skip=skip)
    torch.cuda.synchronize()
    assert a.same_adam(b)
    assert _same_bits(a.ema[dead], e0[dead]) and _same_bits(a.p[dead], p0[dead])
    assert bool((a.ema[~dead] != e0[~dead]).all()) and bool(torch.isfinite(a.ema).all())


# ---- 4. a non-finite gradient -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_non_finite_gradient_leaves_the_average_alone(dev, n):
    p0, grads = _grads(dev, n)
    a = _Set(dev, p0)
    a.step(grads[0], 1e-3, decay=0.9, max_norm=1.0)
    keep = a.snapshot(ema=True)
    g = grads[1].clone()
    g[n - 3] = float("inf")
    a.step(g, 1e-3, decay=0.9, max_norm=1.0)
    assert all(_same_bits(x, y) for x, y in zip(a.snapshot(ema=True), keep))
    assert a.stats[5].item() == 1 and a.stats[3].item() == 2 and a.ticket.item() == 0 and a.state[0].item() == 1
    a.step(grads[1], 1e-3, decay=0.9, max_norm=1.0)
    after = a.snapshot(ema=True)
    assert all(not _same_bits(x, y) for x, y in zip(after, keep))
    assert a.state[0].item() == 2 and a.stats[5].item() == 1 and bool(torch.isfinite(a.ema).all())
    b = _Set(dev, p0)                                                       # (the two finite steps without the bad one in between)
    for g in grads[:2]:
        b.step(g, 1e-3, decay=0.9, max_norm=1.0)
    assert all(_same_bits(x, y) for x, y in zip(after, b.snapshot(ema=True)))


# ---- 5. capture ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_captured_launch_replays_as_three_eager_steps(dev, max_norm):
    from mmego_amd import ops
    n = SIZES[1]
    p0, grads = _grads(dev, n)
    a, b = _Set(dev, p0), _Set(dev, p0)
    for g in grads:
        a.step(g, 1e-3, decay=0.9, max_norm=max_norm)
    torch.cuda.synchronize()
    gbuf = torch.zeros(n, device=dev)
    graph = torch.cuda.CUDAGraph()
    with ops.capture(graph):
        b.step(gbuf, 1e-3, decay=0.9, max_norm=max_norm)
    assert b.state[0].item() == 0 and _same_bits(b.ema, p0)                 # (capturing executes nothing)
    for g in grads:
        gbuf.copy_(g)
        graph.replay()
    assert all(_same_bits(x, y) for x, y in zip(a.snapshot(ema=True), b.snapshot(ema=True)))
    assert torch.equal(a.stats, b.stats) and b.state[0].item() == 3


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    from mmego_amd import hip
    n = 1028
    nb = hip.lib().mmego_grad_norm_nblk(n)
    buf = {k: torch.full((n + 8,), SENTINEL, device=dev) for k in "pgmve"}
    part = torch.full((nb,), SENTINEL, dtype=torch.float64, device=dev)
    state = torch.zeros(3, dtype=torch.float64, device=dev)
    stats = torch.zeros(8, dtype=torch.float64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    p, g, m, v, e = (buf[k] for k in "pgmve")

    def plain(ema, decay):
        hip.call("adam_step_ema", p, g, m, v, n, state, *ADAM, 1e-3, None, 0, ticket, ema, decay)

    def clipped(ema, decay):
        hip.call("adam_step_clipped_ema", p, g, m, v, n, state, *ADAM, 1e-3, None, 0, ticket, part, nb, 1.0, stats, ema, decay)

    for call in (plain, clipped):
        for ema, decay in ((None, 0.9), (e[1:], 0.9), (e, 0.0), (e, 1.0), (e, -0.1), (e, float("nan")), (e, 1.5)):
            with pytest.raises(RuntimeError, match="bad argument"):
                call(ema, decay)
    rc = hip.lib().mmego_adam_step_ema(hip.stream_handle(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr(),
                                       *ADAM, 1e-3, None, 0, ticket.data_ptr(), e.data_ptr(), 0.0)
    assert rc != 0                                                           # (the return code itself)
    torch.cuda.synchronize()
    for t in list(buf.values()) + [part]:
        assert bool((t == SENTINEL).all())
    assert not bool(state.any()) and not bool(stats.any()) and ticket.item() == 0


# ---- 7. FusedAdam -------------------------------------------------------------------------------------------------------------------------------
def test_fused_adam_entry_points_and_never_trained_ranges(dev):
    """On a tiny IMUNet (fc3 never trains: a skip range), as tests/test_clip_grad_norm_gpu.py builds it."""
    from mmego_amd import nets
    from mmego_amd.params import FusedAdam
    from mmego_amd.train_step import empty_step
    torch.manual_seed(7)
    net = nets.IMUNet(15, 9, 32, 2, True, 0).to(dev).train()
    flat = net.flat().ensure()
    off = FusedAdam(net.flat(), lr=1e-3, weight_decay=1e-3)
    assert _entry_points(off.step) == ["adam_step"]                         # (flag off: the launch of today, nothing allocated)
    assert off.ema is None and off.ema_decay is None
    both = FusedAdam(net.flat(), lr=1e-3, weight_decay=1e-3, max_grad_norm=0.5, ema_decay=0.9)
    assert _entry_points(both.step) == ["grad_sqnorm", "adam_step_clipped_ema"]
    opt = FusedAdam(net.flat(), lr=1e-3, weight_decay=1e-3, ema_decay=0.9)
    assert _entry_points(opt.step) == ["adam_step_ema"]
    assert _entry_points(lambda: empty_step(net, opt, None))[-1] == "adam_step_ema"      # (a rank with an empty shard: the same launch)
    dead = torch.zeros(flat.flat_p.numel(), dtype=torch.bool, device=dev)
    for prm, o in zip(flat.params, flat.offsets):
        if any(prm is q for q in net.never_trained()):
            dead[o:o + (prm.numel() + 3) // 4 * 4] = True
    assert bool(dead.any()) and not bool(dead.all())
    before = flat.flat_p.clone()
    assert _same_bits(opt.ema, before) and opt.ema.data_ptr() != flat.flat_p.data_ptr()
    for o in (opt, both):
        flat.flat_p.copy_(before)
        flat.flat_g.copy_(torch.randn(flat.flat_g.numel(), generator=torch.Generator().manual_seed(8)))
        flat.flat_g[dead] = float("nan")
        o.step()
        torch.cuda.synchronize()
        live = ~dead
        for prm, at in zip(flat.params, flat.offsets):                      # (alignment padding between tensors has zero gradient)
            live[at + prm.numel():at + (prm.numel() + 3) // 4 * 4] = False
        assert _same_bits(o.ema[dead], before[dead]) and _same_bits(flat.flat_p[dead], before[dead])
        assert bool((o.ema[live] != before[live]).all()) and bool(torch.isfinite(o.ema).all())
        want = before.double() + (1.0 - 0.9) * (flat.flat_p.double() - before.double())
        assert bool(((o.ema.double() - want).abs()[live] <= EPS * torch.maximum(flat.flat_p.abs(), o.ema.abs()).double()[live]).all())
    sd = opt.state_dict()
    assert sd["ema_decay"] == 0.9 and torch.equal(sd["ema"], opt.ema.cpu())


def _eval_upper(net, batch, R):
    from mmego_amd.train_step import call_upper
    x, _, body, target = batch
    B = x.shape[0]
    z = torch.zeros(6, B, 64, device=x.device)
    with torch.no_grad():
        return call_upper(net.eval(), x.clone(), z, z.clone(), body, R, target[:, :, 20].contiguous())[0].clone()


def _small_batch(dev, B=2, T=4, N=64, seed=42):
    g = torch.Generator().manual_seed(seed)
    batch = [v.to(dev) for v in (torch.randn(B, T, N, 6, generator=g), torch.randn(B, T, 20, 15, generator=g),
                                 torch.randn(B, 20, 3, generator=g) * 0.3, torch.randn(B, T, 21, 3, generator=g))]
    R = torch.linalg.qr(torch.randn(B, T, 3, 3, generator=g))[0].contiguous().to(dev)
    return batch, R


def _averaged_round_trip(opt, net, forward, fresh):
    """forward(net) before, inside and after averaged(); ``fresh``: a second instance, which gets ema_state_dict()."""
    f = net.flat()
    raw = f.flat_p.clone()
    y_raw = forward(net)                                                     # (leaves whatever the net derives from the RAW weights behind)
    fresh.load_state_dict(opt.ema_state_dict())
    y_fresh = forward(fresh)
    with opt.averaged():
        y_avg = forward(net)
        assert not _same_bits(f.flat_p, raw)
        with pytest.raises(RuntimeError, match="not re-entrant"):
            with opt.averaged():
                pass
        with pytest.raises(RuntimeError, match="inside averaged"):
            opt.step()
    assert _same_bits(y_avg, y_fresh)
    assert not _same_bits(y_avg, y_raw)
    assert _same_bits(f.flat_p, raw) and _same_bits(forward(net), y_raw)


def test_averaged_upper_net(dev):
    from mmego_amd import nets
    from mmego_amd.train_step import StageStep
    batch, R = _small_batch(dev)
    torch.manual_seed(41)
    net = nets.UpperNet().to(dev).train()
    st = StageStep("upper", net, None, lr=1e-3, use_graph=False, ema_decay=0.5)
    st.bind(*batch, R_gt=R)
    for _ in range(3):
        st.step()
    torch.cuda.synchronize()
    _averaged_round_trip(st.opt, net, lambda m: _eval_upper(m, batch, R), nets.UpperNet().to(dev))


def test_averaged_imu_net_in_split3_mode(dev):
    """precision = "split3" keeps bf16 pieces of the LSTM weights: both exchanges have to drop them (hidden size 256, B=4, T=8: the smallest
    shape the mode takes)."""
    from mmego_amd import nets
    from mmego_amd.train_step import ImuStep
    batch, R = _small_batch(dev, B=4, T=8)
    torch.manual_seed(43)
    net = nets.IMUNet(15, 9, 256, 2, True, 0).to(dev).train()
    st = ImuStep(net, lr=1e-3, use_graph=False, ema_decay=0.5)
    st.bind(batch[1], R, batch[3])
    for _ in range(3):
        st.step()
    torch.cuda.synchronize()
    fresh = nets.IMUNet(15, 9, 256, 2, True, 0).to(dev)
    net.precision = fresh.precision = "split3"

    def forward(m):
        with torch.no_grad():
            Rm, tm = m.eval()(batch[1])
            return torch.cat((Rm.reshape(-1), tm.reshape(-1))).clone()
    _averaged_round_trip(st.opt, net, forward, fresh)


# ---- 8. the step engines --------------------------------------------------------------------------------------------------------------------
def _make_step(dev, kind, use_graph, decay, batch, R):
    from mmego_amd import nets
    from mmego_amd.train_step import ImuStep, StageStep
    torch.manual_seed(41)
    up = nets.UpperNet().to(dev).train()
    imu = nets.IMUNet(15, 9, 64, 2, True, 0).to(dev).train()
    if kind == "imu":
        st = ImuStep(imu, lr=1e-4, use_graph=use_graph, ema_decay=decay)
        st.bind(batch[1], R, batch[3])
    else:
        fine = kind == "finetune_imu"
        st = StageStep("upper", up, imu if fine else None, lr=3e-5, use_graph=use_graph, finetune_imu=fine, imu_lr=1e-5, ema_decay=decay)
        st.bind(*batch, R_gt=None if fine else R)
    return st


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("kind", ["upper", "imu", "finetune_imu"])
def test_steps_keep_their_parameters_and_average_each_net(dev, kind, use_graph):
    batch, R = _small_batch(dev)
    a, b = _make_step(dev, kind, use_graph, 0.9, batch, R), _make_step(dev, kind, use_graph, None, batch, R)
    opts_a, opts_b = a.optimisers(), b.optimisers()
    assert len(opts_a) == (2 if kind == "finetune_imu" else 1)
    assert all(o.ema_decay == 0.9 for o in opts_a) and all(o.ema_decay is None and o.ema is None for o in opts_b)
    start = [o.flat.ensure().flat_p.clone() for o in opts_a]
    ps, es = [[] for _ in opts_a], [[] for _ in opts_a]
    for step in range(3):
        la, lb = a.step().clone(), b.step().clone()
        torch.cuda.synchronize()
        assert torch.equal(la, lb), step
        for i, (oa, ob) in enumerate(zip(opts_a, opts_b)):
            assert _same_bits(oa.flat.flat_p, ob.flat.flat_p), (step, i)
            assert _same_bits(oa.m, ob.m) and _same_bits(oa.v, ob.v) and torch.equal(oa.state, ob.state), (step, i)
            ps[i].append(oa.flat.flat_p.clone())
            es[i].append(oa.ema.clone())
    assert all(o.ema is None for o in opts_b)
    for i, oa in enumerate(opts_a):
        assert oa.ema.numel() == oa.flat.flat_p.numel() and not _same_bits(oa.ema, oa.flat.flat_p)
        _check_recurrence(start[i], ps[i], es[i], 0.9, "%s graph=%s optimiser %d" % (kind, use_graph, i))
    if kind == "finetune_imu":
        assert opts_a[0].flat.module is a.net and opts_a[1].flat.module is a.imu and opts_a[0].ema.numel() != opts_a[1].ema.numel()


# ---- 9. the command line --------------------------------------------------------------------------------------------------------------------
START = "[mmego_amd] weight averaging: decay 0.9; evaluation and early stopping use the averaged weights"


def _ckpt(out_dir, idx, epoch, sub=""):
    f = [f for f in glob.glob(os.path.join(out_dir, "model", str(idx), sub, "epoch%d_*.pth" % epoch)) if not f.endswith(".train_state.pth")]
    assert len(f) == 1, f
    return f[0]


def _equal_ckpt(a, b):
    sa, sb = torch.load(a, map_location="cpu"), torch.load(b, map_location="cpu")
    assert sa.keys() == sb.keys()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


def test_cli_upper_net_two_epochs_equal_one_plus_resume(tmp_path):
    """--train --network Upper_Net --ema_decay 0.9: two epochs in one go against one epoch and --resume WITHOUT the flag (the optimiser
    state carries the average and its decay): the raw checkpoint, the EMA/ file and the state's average are equal; the EMA/ file is a
    reference-format Upper_Net checkpoint that differs from the raw one."""
    from mmego_amd import nets
    from test_cli_gpu import _make_dataset, _run
    data = str(tmp_path / "Sample_data")
    _make_dataset(data, np.random.default_rng(1))
    out_dir = str(tmp_path / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    base = ["--train", "--network", "Upper_Net", "--gt_head_pose", "--data_root", data, "--batch_size", "4", "--device", "cuda:0", "--seed", "5"]
    out = _run(base + ["--ema_decay", "0.9", "--epochs", "2", "--log_dir", "9171"], env)
    assert out.count(START) == 1
    out = _run(base + ["--ema_decay", "0.9", "--epochs", "1", "--log_dir", "9172"], env)
    assert out.count(START) == 1
    first = _ckpt(out_dir, 9172, 0)
    assert os.path.exists(_ckpt(out_dir, 9172, 0, "EMA"))
    out = _run(base + ["--epochs", "2", "--log_dir", "9173", "--resume", first], env)
    assert "resumed from" in out and "epoch: 2" in out and "epoch: 1\n" not in out and out.count(START) == 1
    assert "restarts" not in out
    a, b = _ckpt(out_dir, 9171, 1), _ckpt(out_dir, 9173, 1)
    ea, eb = _ckpt(out_dir, 9171, 1, "EMA"), _ckpt(out_dir, 9173, 1, "EMA")
    assert os.path.basename(ea) == os.path.basename(a)
    assert _equal_ckpt(a, b) and _equal_ckpt(ea, eb)
    ta = torch.load(a[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)
    tb = torch.load(b[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)
    for k in ("m", "v", "state", "ema"):
        assert torch.equal(ta["optimizer"][k], tb["optimizer"][k]), k
    assert ta["optimizer"]["ema_decay"] == tb["optimizer"]["ema_decay"] == 0.9
    raw, avg = torch.load(a, map_location="cpu"), torch.load(ea, map_location="cpu")
    assert all(torch.equal(ta["model"][k], raw[k]) for k in raw)            # (the train state keeps the RAW weights)
    fresh = nets.UpperNet()
    fresh.load_state_dict(avg)                                              # (strict: every key, every shape)
    params = [k for k, _ in fresh.named_parameters()]
    assert raw.keys() == avg.keys() and any(not torch.equal(raw[k], avg[k]) for k in params)
    assert all(torch.equal(raw[k], avg[k]) for k in raw if k not in params)  # (buffers are not averaged: the live ones)
    assert all(bool(torch.isfinite(avg[k]).all()) for k in params)
