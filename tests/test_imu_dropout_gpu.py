"""GPU: IMU_Net training with nn.LSTM(dropout=p) between the layers of its two BiLSTM(512) stacks (--imu_dropout).

The masks are counter-based (csrc/common.h): element i of a launch is kept when a 24-bit hash of (i, key(seed word, salt)) is >= p.  The
first test restates that hash in numpy and holds mmego_lstm_dropout to it bit for bit; the net tests then take the KERNEL's masks (the
launch on ones) into a float64 reference, so they need no statistical bar.

Bars of the net tests: tests/test_hip_local.py::test_imu_stage1_gradients_at_full_size's -- outputs atol 2e-5, every gradient element
within 2e-4 of the largest gradient."""
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from oracle import geometry as geo
from oracle import nets as on

pytestmark = pytest.mark.gpu

GRAD_BAR = 2e-4
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
DEFAULT_WORD = 0x9E3779B97F4A7C15 & 0x7FFFFFFFFFFFFFFF
SENTINEL = -7.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


# ---- the hash of csrc/common.h, restated on the host (uint32 arithmetic, float32 compare) ---------------------------------------------
def _hash32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def _dropout_key(seed, salt):
    seed = ((seed + salt * 0x9E3779B97F4A7C15) * 6364136223846793005 + 1442695040888963407) & M64
    return int(_hash32(np.array([((seed & M32) + 0x9e3779b9 * (seed >> 32)) & M32], dtype=np.uint32))[0])


def _host_mask(seed, salt, n, p):
    """m(i), i < n: 0 or float32(1 / (1 - p)) (fp32 arithmetic as in the kernel)."""
    i = np.arange(n, dtype=np.uint32)
    u = (_hash32(i ^ np.uint32(_dropout_key(seed, salt))) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    keep = u >= np.float32(p)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(keep, scale, np.float32(0.0)).astype(np.float32)


def _lcg(word):
    return (word * 6364136223846793005 + 1442695040888963407) & M64


def _word(t):
    return int(t.item()) & M64


def _seed(dev, value):
    return torch.tensor([value if value < (1 << 63) else value - (1 << 64)], dtype=torch.int64, device=dev)


def _layout(dev, x, kind):
    """x [rows, cols] (host) as a device operand of the given layout in a sentinel-filled buffer -> (view, whole buffer).
    dense: ld = cols, aligned; dense1: ld = cols, base one float past an aligned address; wide: ld = cols + 4, aligned (16-byte path with
    a leading dimension); slice: ld = cols + 3, base one float past an aligned address (the dword path)."""
    rows, cols = x.shape
    ld, lead = {"dense": (cols, 0), "dense1": (cols, 1), "wide": (cols + 4, 0), "slice": (cols + 3, 1)}[kind]
    buf = torch.full((lead + rows * ld + 64,), SENTINEL, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[lead:lead + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(x.to(dev))
    return view, buf


def _bits(t):
    return t.contiguous().cpu().view(torch.int32)


def _outside(buf, view):
    """The sentinel positions of a _layout buffer (everything that is not the view)."""
    mark = torch.zeros_like(buf, dtype=torch.bool)
    rows, cols = view.shape
    lead = (view.data_ptr() - buf.data_ptr()) // 4
    mark[lead:lead + rows * view.stride(0)].view(rows, view.stride(0))[:, :cols] = True
    return buf[~mark]


@pytest.mark.parametrize("rows,cols", [(3, 8), (65, 128), (257, 1024), (1280, 1024)])
def test_kernel_against_host_restatement(dev, rows, cols):
    """Y == X * m bit for bit (one fp32 multiply), m in {0, float32(1/(1-p))} from the numpy hash at the LOGICAL index r * cols + c,
    whatever the leading dimensions: dense and strided operands, 16-byte and dword paths, out of place and in place, nothing written
    outside Y."""
    from mmego_amd import ops
    gen = torch.Generator().manual_seed(rows * 7 + cols)
    x = torch.randn(rows, cols, generator=gen)
    seed = _seed(dev, 12345)
    for p in (0.1, 0.5):
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        for salt in (0, 1, 8, 9):
            m = _host_mask(12345, salt, rows * cols, p).reshape(rows, cols)
            assert set(np.unique(m).tolist()) <= {0.0, float(scale)}
            want = torch.from_numpy(x.numpy() * m)
            for kind in ("dense", "slice", "wide", "dense1"):
                xv, xbuf = _layout(dev, x, kind)
                yv, ybuf = _layout(dev, torch.full((rows, cols), SENTINEL), kind)
                ops.lstm_dropout(xv, yv, p, seed, salt)                       # out of place
                assert torch.equal(_bits(yv), _bits(want)), (p, salt, kind)
                assert bool((_outside(ybuf, yv) == SENTINEL).all()), (p, salt, kind)
                assert torch.equal(_bits(xv), _bits(x))
                ops.lstm_dropout(xv, xv, p, seed, salt)                       # in place
                assert torch.equal(_bits(xv), _bits(want)), (p, salt, kind, "in place")
                assert bool((_outside(xbuf, xv) == SENTINEL).all()), (p, salt, kind, "in place")
    assert _word(seed) == 12345                                                # (the word is only read)


def test_kernel_mixed_layouts(dev):
    """A dense source into a column slice and back (the two leading dimensions differ)."""
    from mmego_amd import ops
    rows, cols, p, salt = 65, 128, 0.1, 9
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(5))
    want = torch.from_numpy(x.numpy() * _host_mask(12345, salt, rows * cols, p).reshape(rows, cols))
    seed = _seed(dev, 12345)
    for kx, ky in (("dense", "slice"), ("slice", "dense"), ("dense", "wide"), ("wide", "dense1")):
        xv, _ = _layout(dev, x, kx)
        yv, ybuf = _layout(dev, torch.full((rows, cols), SENTINEL), ky)
        ops.lstm_dropout(xv, yv, p, seed, salt)
        assert torch.equal(_bits(yv), _bits(want)), (kx, ky)
        assert bool((_outside(ybuf, yv) == SENTINEL).all()), (kx, ky)


def test_one_mask_convention_across_both_kernels(dev):
    """The mask of (512, 128), seed 12345, salt 0, p 0.1 is the one mmego_lstm64_forward stores for its layer 0 (the setup of
    tests/test_hip_parity.py::test_lstm64_fused_dropout_and_bias_pair); two salts, and the word before and after a seed_take, differ."""
    from mmego_amd import blocks, ops
    torch.manual_seed(3)
    lstm = blocks.LstmParams(64, 64, 3, dropout=0.1).to(dev)
    B, T, p = 64, 8, 0.1
    x = torch.randn(B * T, 64, device=dev)
    seed = _seed(dev, 12345)
    ar = ops.Arena(dev)
    blocks.lstm64_forward(ar, "k", lstm, x, B, T, None, None, True, p, seed)
    ones = torch.ones(B * T, 128, device=dev)
    m = [ops.lstm_dropout(ones, torch.empty_like(ones), p, seed, salt) for salt in (0, 1)]
    assert torch.equal(m[0], ar.get("k.mk0", (B * T, 128))) and torch.equal(m[1], ar.get("k.mk1", (B * T, 128)))
    assert torch.equal(m[0].cpu(), torch.from_numpy(_host_mask(12345, 0, B * T * 128, p).reshape(B * T, 128)))
    assert not torch.equal(m[0], m[1])
    taken = torch.zeros(1, dtype=torch.int64, device=dev)
    ops.seed_take(seed, taken)
    after = ops.lstm_dropout(ones, torch.empty_like(ones), p, seed, 0)
    assert not torch.equal(after, m[0])
    assert torch.equal(ops.lstm_dropout(ones, torch.empty_like(ones), p, taken, 0), m[0])      # (the taken word keeps the old masks)


def test_drop_rate(dev):
    """(1280, 1024) draws: the fraction of zeros within 4 sigma of p, sigma = sqrt(p (1 - p) / n) -- a condition on the hash, for the
    seed words 12345, 12346 and the nets' default word, salts 0, 1, 8, 9, both rates.  (The numpy restatement gives at most 2.42 sigma
    over these cases and three shapes.)"""
    from mmego_amd import ops
    rows, cols = 1280, 1024
    n = rows * cols
    ones = torch.ones(rows, cols, device=dev)
    y = torch.empty_like(ones)
    for word in (12345, 12346, DEFAULT_WORD):
        seed = _seed(dev, word)
        for p in (0.1, 0.5):
            sigma = (p * (1 - p) / n) ** 0.5
            for salt in (0, 1, 8, 9):
                rate = float((ops.lstm_dropout(ones, y, p, seed, salt) == 0).double().mean())
                print("drop rate: word %d p %.1f salt %d: %.6f (%.2f sigma)" % (word, p, salt, rate, abs(rate - p) / sigma))
                assert abs(rate - p) < 4 * sigma, (word, p, salt, rate, sigma)


def test_refusals_launch_nothing(dev):
    """cols = 6, p = 0, p = 1: a status (the wrapper raises) and Y keeps its sentinel."""
    from mmego_amd import ops
    seed = _seed(dev, 12345)
    for cols, p in ((6, 0.1), (8, 0.0), (8, 1.0)):
        x = torch.randn(5, cols, device=dev)
        y = torch.full((5, cols), SENTINEL, device=dev)
        with pytest.raises(RuntimeError, match="mmego_lstm_dropout failed: bad argument"):
            ops.lstm_dropout(x, y, p, seed, 0)
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all()), (cols, p)
    from mmego_amd import hip
    x = torch.randn(5, 8, device=dev)
    for ldx, ldy, word in ((4, 8, seed), (8, 4, seed), (8, 8, None)):        # a leading dimension below cols; no seed word
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("lstm_dropout", x, ldx, x, ldy, 5, 8, 0.1, word, 0)
    # in place is X == Y with ONE leading dimension; any other overlap of the operands would race between lanes and is refused
    buf = torch.full((200,), SENTINEL, device=dev)
    for xo, ldx, yo, ldy in ((0, 8, 0, 12), (0, 12, 0, 8), (0, 8, 4, 8), (8, 8, 0, 8), (0, 8, 36, 8)):
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("lstm_dropout", buf[xo:], ldx, buf[yo:], ldy, 5, 8, 0.1, seed, 0)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    hip.call("lstm_dropout", buf, 8, buf[40:], 8, 5, 8, 0.1, seed, 0)        # (neighbours that only touch are fine)


def test_seed_take(dev):
    """taken is the old word; the counter afterwards is the one an inc_i64 leaves from the same start (words with the top bit set too)."""
    from mmego_amd import hip, ops
    for start in (12345, DEFAULT_WORD, _lcg(DEFAULT_WORD), M64):
        ctr, ref = _seed(dev, start), _seed(dev, start)
        taken = torch.zeros(1, dtype=torch.int64, device=dev)
        ops.seed_take(ctr, taken)
        hip.call("inc_i64", None, 0, ref)
        assert _word(taken) == start
        assert torch.equal(ctr, ref) and _word(ctr) == _lcg(start)


# ---- the net ---------------------------------------------------------------------------------------------------------------------------
def _nets(dev, H, p, seed):
    from mmego_amd import nets
    torch.manual_seed(seed)
    o = on.IMUNet(15, 9, H, 2, True, p)
    hb = nets.IMUNet(15, 9, H, 2, True, p)
    hb.load_state_dict(o.state_dict())
    return o, hb.to(dev).train()


def _one_layer(o_lstm, l):
    """Layer l of a two-layer bidirectional nn.LSTM as a one-layer float64 module."""
    In = o_lstm.input_size if l == 0 else 2 * o_lstm.hidden_size
    m = torch.nn.LSTM(In, o_lstm.hidden_size, 1, bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            for sfx in ("", "_reverse"):
                getattr(m, "%s_l0%s" % (kind, sfx)).copy_(getattr(o_lstm, "%s_l%d%s" % (kind, l, sfx)).double())
    return m


def _reference_f64(o, imu, masks, wR, wt):
    """oracle.nets.IMUNet.forward in float64 with each stack as two one-layer modules and the given masks in between ->
    (R, t, {parameter name: gradient})."""
    lin = {}
    for name in ("fc1", "fc2", "attn"):
        src = getattr(o, name)
        lin[name] = torch.nn.Linear(src.in_features, src.out_features).double()
        lin[name].load_state_dict({k: v.double() for k, v in src.state_dict().items()})
    layers = {s: [_one_layer(getattr(o, s), l) for l in (0, 1)] for s in ("rnn_fast", "rnn_slow")}
    B, T, S, _ = imu.shape
    x = torch.relu(lin["fc1"](imu.double().reshape(B * T, S, -1)))
    f0, _ = layers["rnn_fast"][0](x)
    fast, _ = layers["rnn_fast"][1](f0 * masks[0].double().view(B * T, S, -1))
    w = torch.softmax(lin["attn"](fast), dim=1)
    pooled = (fast * w).sum(dim=1).view(B, T, -1)
    s0, _ = layers["rnn_slow"][0](pooled)
    slow, _ = layers["rnn_slow"][1](s0 * masks[1].double().view(B, T, -1))
    out = lin["fc2"](slow).reshape(B * T, -1)
    R = geo.rot6d_imu(out[:, :6]).view(B, T, 3, 3)
    t = out[:, 6:].reshape(B, T, 3)
    ((R * wR.double()).sum() + (t * wt.double()).sum()).backward()
    grads = {}
    for name, m in lin.items():
        for k, prm in m.named_parameters():
            grads["%s.%s" % (name, k)] = prm.grad
    for s, pair in layers.items():
        for l, m in enumerate(pair):
            for k, prm in m.named_parameters():
                grads["%s.%s" % (s, k.replace("_l0", "_l%d" % l))] = prm.grad
    return R.detach(), t.detach(), grads


def _kernel_masks(dev, word, p, Bn, S, B, T, H):
    """The masks a training forward with seed word `word` applies: rnn_fast's layer 0 (salt 0) and rnn_slow's (salt 8)."""
    from mmego_amd import ops
    out = []
    for rows, salt in ((Bn * S, 0), (B * T, 8)):
        ones = torch.ones(rows, 2 * H, device=dev)
        out.append(ops.lstm_dropout(ones, torch.empty_like(ones), p, word, salt).cpu())
    return out


@pytest.mark.parametrize("H,B,T", [(32, 3, 4), (512, 16, 8)])
def test_net_against_float64_with_the_kernels_masks(dev, H, B, T):
    """IMUNet(15, 9, H, 2, True, 0.25).train(): forward and every gradient against float64 (H = 512, 128 rnn_fast rows: the full-size
    dispatch -- lstm_step_dma, lstm_bwd_step)."""
    p, S = 0.25, 20
    o, hb = _nets(dev, H, p, 31)
    gen = torch.Generator().manual_seed(100 + B)
    imu = torch.randn(B, T, S, 15, generator=gen)
    wR, wt = torch.randn(B, T, 3, 3, generator=gen), torch.randn(B, T, 3, generator=gen)
    word = hb.seed_counter().clone()
    masks = _kernel_masks(dev, word, p, B * T, S, B, T, H)
    for m in masks:
        assert 0.2 < float((m == 0).float().mean()) < 0.3
    Ro, to_, go = _reference_f64(o, imu, masks, wR, wt)
    Rh, th = hb(imu.to(dev))
    ((Rh * wR.to(dev)).sum() + (th * wt.to(dev)).sum()).backward()
    assert _word(hb.seed_counter()) == _lcg(_word(word))
    eR, et = float((Rh.detach().double().cpu() - Ro).abs().max()), float((th.detach().double().cpu() - to_).abs().max())
    print("imu dropout H=%d: outputs off by %.3e (R) %.3e (t)" % (H, eR, et))
    assert eR < 2e-5 and et < 2e-5, (eR, et)
    scale = max(float(g.abs().max()) for g in go.values())
    worst = 0.0
    for k, ph in hb.named_parameters():
        if k.startswith("fc3."):
            assert ph.grad is None or not bool(ph.grad.any()), k
            continue
        err = float((ph.grad.double().cpu() - go[k]).abs().max())
        worst = max(worst, err)
        assert err < GRAD_BAR * scale, (H, k, err, scale)
    print("imu dropout H=%d: gradients, worst error %.3e at scale %.3e (%.2e of it)" % (H, worst, scale, worst / scale))
    assert set(go) == {k for k, _ in hb.named_parameters() if not k.startswith("fc3.")}


def _body_grads(hb, imu, dR, dt):
    """One training forward + backward on the kernel pipelines (no autograd) -> (R, t, flat gradient)."""
    from mmego_amd import imu_train
    hb.flat().flat_g.zero_()
    with torch.no_grad():
        R, t = imu_train.forward_train(hb, imu)
        imu_train.backward(hb, dR, dt)
    torch.cuda.synchronize()
    return R.clone(), t.clone(), hb.flat().flat_g.clone()


def test_split3_on_top_of_dropout(dev):
    """H = 512, (64, 8), train_precision "split3" against the fp32 run from the same counter value: the masks are bit-equal by
    construction, the products are the only difference."""
    from mmego_amd import hip
    from mmego_amd.plan import StepPlan
    B, T = 64, 8
    _, hb = _nets(dev, 512, 0.25, 33)
    gen = torch.Generator().manual_seed(7)
    imu = torch.randn(B, T, 20, 15, generator=gen).to(dev)
    dR, dt = torch.randn(B, T, 3, 3, generator=gen).to(dev), torch.randn(B, T, 3, generator=gen).to(dev)
    start = hb.seed_counter().clone()
    res = {}
    for prec in ("fp32", "split3"):
        hb.train_precision = prec
        hb.seed_counter().copy_(start)
        res[prec] = _body_grads(hb, imu, dR, dt)
    from mmego_amd import imu_train
    hb.seed_counter().copy_(start)
    with torch.no_grad():
        plan = StepPlan().record(lambda: (imu_train.forward_train(hb, imu), imu_train.backward(hb, dR, dt)))
    names = [n for sg in plan.segments for n, _ in sg.calls]
    assert sum(hip.is_bf16_mfma_entry(n) for n in names) >= 8 and names.count("lstm_dropout") == 4 and names.count("seed_take") == 1
    a, b = res["fp32"][2], res["split3"][2]
    scale, err = float(a.abs().max()), float((a - b).abs().max())
    print("imu dropout split3 vs fp32: gradients %.3e at scale %.3e" % (err, scale))
    assert err < GRAD_BAR * scale, (err, scale)
    assert not torch.equal(a, b)


def test_counter_semantics(dev):
    from mmego_amd import hip, imu_train, nets
    from mmego_amd.plan import StepPlan
    B, T = 3, 4
    o, hb = _nets(dev, 32, 0.25, 35)
    plain = nets.IMUNet(15, 9, 32, 2, True, 0)
    plain.load_state_dict(o.state_dict())
    plain = plain.to(dev).train()
    gen = torch.Generator().manual_seed(8)
    imu = torch.randn(B, T, 20, 15, generator=gen).to(dev)
    dR, dt = torch.randn(B, T, 3, 3, generator=gen).to(dev), torch.randn(B, T, 3, generator=gen).to(dev)
    start = hb.seed_counter().clone()
    # two training forwards in a row: other masks, one inc_i64 step of the counter each
    r1 = _body_grads(hb, imu, dR, dt)
    assert _word(hb.seed_counter()) == _lcg(_word(start))
    r2 = _body_grads(hb, imu, dR, dt)
    assert _word(hb.seed_counter()) == _lcg(_lcg(_word(start)))
    assert not torch.equal(r1[0], r2[0]) and not torch.equal(r1[2], r2[2])
    # the counter put back: the same bits
    hb.seed_counter().copy_(start)
    r3 = _body_grads(hb, imu, dR, dt)
    for a, b in zip(r1, r3):
        assert torch.equal(a, b)
    # eval: the dropout-free net's forward, counter left alone
    hb.eval(), plain.eval()
    before = hb.seed_counter().clone()
    with torch.no_grad():
        Re, te = hb(imu)
        Rp, tp = plain(imu)
    assert torch.equal(Re, Rp) and torch.equal(te, tp) and torch.equal(hb.seed_counter(), before)
    hb.train(), plain.train()
    # lstm_dropout = 0 overrides the constructor's rate: the dropout-free net's step, neither new entry point, counter left alone
    hb.lstm_dropout = 0
    r4 = _body_grads(hb, imu, dR, dt)
    rp = _body_grads(plain, imu, dR, dt)
    for a, b in zip(r4, rp):
        assert torch.equal(a, b)
    assert torch.equal(hb.seed_counter(), before)
    with torch.no_grad():
        plan = StepPlan().record(lambda: (imu_train.forward_train(hb, imu), imu_train.backward(hb, dR, dt)))
    names = [n for sg in plan.segments for n, _ in sg.calls]
    assert "lstm_dropout" not in names and "seed_take" not in names
    hb.lstm_dropout = None
    with torch.no_grad():
        plan = StepPlan().record(lambda: (imu_train.forward_train(hb, imu), imu_train.backward(hb, dR, dt)))
    names = [n for sg in plan.segments for n, _ in sg.calls]
    assert names.count("lstm_dropout") == 4 and names.count("seed_take") == 1 and names.index("seed_take") < names.index("lstm_dropout")
    # a stack of one layer has no layer output to drop: nothing is launched for it and no seed word is taken
    single = nets.IMUNet(15, 9, 32, 1, True, 0.25).to(dev).train()
    word1 = single.seed_counter().clone()
    with torch.no_grad():
        plan = StepPlan().record(lambda: (imu_train.forward_train(single, imu), imu_train.backward(single, dR, dt)))
    names = [n for sg in plan.segments for n, _ in sg.calls]
    assert "lstm_dropout" not in names and "seed_take" not in names
    _body_grads(single, imu, dR, dt)
    assert torch.equal(single.seed_counter(), word1)
    # a rate outside [0, 1) is refused at the training forward, before anything is launched
    for bad in (1.0, -0.1):
        hb.lstm_dropout = bad
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            hb(imu)
        seen, orig = [], hip._launch
        hip._launch = lambda name, *a: seen.append(name)
        try:
            with pytest.raises(ValueError, match=r"\[0, 1\)"):
                imu_train.forward_train(hb, imu)
        finally:
            hip._launch = orig
        assert seen == []
    hb.lstm_dropout = None


def _three_steps(make, use_graph):
    st = make(use_graph)
    start = _word(st_imu(st).seed_counter())
    losses = [st.step().item() for _ in range(3)]
    torch.cuda.synchronize()
    assert (st.graph is not None) == use_graph
    assert _word(st_imu(st).seed_counter()) == _lcg(_lcg(_lcg(start)))           # three forwards; the warm-up left no trace
    nets_ = [st.net] + ([st.imu] if getattr(st, "imu", None) is not None else [])
    return losses, [(n.flat().flat_g.clone(), n.flat().flat_p.clone()) for n in nets_]


def st_imu(st):
    return st.imu if getattr(st, "imu", None) is not None else st.net


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for (ga, pa), (gb, pb) in zip(a[1], b[1]):
        assert torch.equal(ga, gb) and torch.equal(pa, pb)


def test_imu_step_eager_equals_graph(dev):
    """ImuStep with an IMU_Net built with 0.1 (H = 512, B = 4, T = 8): three steps eager and three from the graph, same start."""
    from mmego_amd import nets
    from mmego_amd.train_step import ImuStep
    B, T = 4, 8
    torch.manual_seed(41)
    sd = {k: v.clone() for k, v in nets.IMUNet(15, 9, 512, 2, True, 0.1).state_dict().items()}
    g = torch.Generator().manual_seed(42)
    imu = torch.randn(B, T, 20, 15, generator=g).to(dev)
    tgt = torch.randn(B, T, 21, 3, generator=g).to(dev)
    R = geo.rot6d_imu(torch.randn(B * T, 6, generator=g)).view(B, T, 3, 3).contiguous().to(dev)

    def make(use_graph, drop=None):
        net = nets.IMUNet(15, 9, 512, 2, True, 0.1)
        net.load_state_dict(sd)
        net = net.to(dev).train()
        net.lstm_dropout = drop
        st = ImuStep(net, use_graph=use_graph)
        st.bind(imu, R, tgt)
        return st
    eager, graph = _three_steps(make, False), _three_steps(make, True)
    _same(eager, graph)
    assert all(np.isfinite(eager[0]))
    off = make(True, drop=0)
    off.step()
    torch.cuda.synchronize()
    one = make(True)
    one.step()
    torch.cuda.synchronize()
    assert not torch.equal(one.net.flat().flat_g, off.net.flat().flat_g)         # the masks are live in the captured graph


def test_finetune_stage_eager_equals_graph(dev):
    """StageStep("upper", ..., finetune_imu=True) with an IMU_Net built with 0.1 (B = 4, T = 8, N = 128)."""
    from mmego_amd import nets
    from mmego_amd.train_step import StageStep
    B, T, N = 4, 8, 128
    torch.manual_seed(41)
    sd_imu = {k: v.clone() for k, v in nets.IMUNet(15, 9, 512, 2, True, 0.1).state_dict().items()}
    sd_up = {k: v.clone() for k, v in nets.UpperNet().state_dict().items()}
    g = torch.Generator().manual_seed(42)
    batch = [v.to(dev) for v in (torch.randn(B, T, N, 6, generator=g), torch.randn(B, T, 20, 15, generator=g),
                                 torch.randn(B, 20, 3, generator=g) * 0.3, torch.randn(B, T, 21, 3, generator=g))]

    def make(use_graph, drop=None):
        himu = nets.IMUNet(15, 9, 512, 2, True, 0.1)
        himu.load_state_dict(sd_imu)
        himu = himu.to(dev).train()
        himu.lstm_dropout = drop
        hup = nets.UpperNet()
        hup.load_state_dict(sd_up)
        hup = hup.to(dev).train()
        st = StageStep("upper", hup, himu, lr=3e-5, use_graph=use_graph, finetune_imu=True, imu_lr=1e-5)
        st.bind(*batch)
        return st
    eager, graph = _three_steps(make, False), _three_steps(make, True)
    _same(eager, graph)
    assert all(np.isfinite(eager[0]))
    off = make(True, drop=0)
    off.step()
    one = make(True)
    one.step()
    torch.cuda.synchronize()
    assert not torch.equal(one.imu.flat().flat_g, off.imu.flat().flat_g)         # the masks are live in the captured graph


def test_default_imu_step_is_unchanged(dev):
    """ImuStep._body for a dropout = 0 net (B = 4, T = 8) launches exactly what it launched before IMU_Net training had dropout
    (tests/golden/imu_step_entry_points.json: recorded on the commit before this feature), keeps no dropped copy and no taken word, and
    does not touch the counter.  To record the file again: check out the commit before this feature, build it, run this test's set-up
    (seeds 3 and 4, one eager step) there and dump {"entry_points": [n for sg in StepPlan().record(st._body).segments for n, _ in
    sg.calls]} as JSON."""
    from mmego_amd import nets
    from mmego_amd.plan import StepPlan
    from mmego_amd.train_step import ImuStep
    B, T = 4, 8
    torch.manual_seed(3)
    net = nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).train()
    g = torch.Generator().manual_seed(4)
    imu = torch.randn(B, T, 20, 15, generator=g).to(dev)
    tgt = torch.randn(B, T, 21, 3, generator=g).to(dev)
    R = geo.rot6d_imu(torch.randn(B * T, 6, generator=g)).view(B, T, 3, 3).contiguous().to(dev)
    before = net.seed_counter().clone()
    st = ImuStep(net, use_graph=False)
    st.bind(imu, R, tgt)
    st.step()
    torch.cuda.synchronize()
    names = [n for sg in StepPlan().record(st._body).segments for n, _ in sg.calls]
    want = json.load(open(os.path.join(GOLDEN, "imu_step_entry_points.json")))
    assert names == want["entry_points"], [(i, a, b) for i, (a, b) in enumerate(zip(names, want["entry_points"])) if a != b][:5]
    assert "lstm_dropout" not in names and "seed_take" not in names
    assert not any(k[0] == "drop.word" or re.search(r"\.do\d+$", k[0]) for k in net.arena("train").bufs)
    assert torch.equal(net.seed_counter(), before)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_tree(tmp_path_factory):
    """The synthetic tree of tests/test_cli_gpu.py and ONE stage-1 epoch with --imu_dropout 0.1 that the tests below share."""
    from test_cli_gpu import _make_dataset, _run
    tmp = tmp_path_factory.mktemp("imu_dropout_cli")
    data = str(tmp / "Sample_data")
    _make_dataset(data, np.random.default_rng(1))
    out_dir = str(tmp / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    base = ["--train", "--network", "IMU_Net", "--data_root", data, "--batch_size", "4", "--device", "cuda:0", "--seed", "0"]
    _run(base + ["--imu_dropout", "0.1", "--epochs", "1", "--log_dir", "9151"], env)
    return dict(tmp=tmp, data=data, out_dir=out_dir, env=env, base=base, run=_run)


def _ckpt(out_dir, idx, epoch):
    f = [f for f in glob.glob(os.path.join(out_dir, "model", str(idx), "epoch%d_*.pth" % epoch)) if not f.endswith(".train_state.pth")]
    assert len(f) == 1, f
    return f[0]


def _equal_ckpt(a, b):
    sa, sb = torch.load(a, map_location="cpu"), torch.load(b, map_location="cpu")
    assert sa.keys() == sb.keys()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


def test_cli_stage1_dropout_is_reproducible_and_live(cli_tree):
    """--train --network IMU_Net --imu_dropout 0.1 --epochs 1 --seed 0 twice: equal checkpoints; without the flag: another one."""
    c = cli_tree
    c["run"](c["base"] + ["--imu_dropout", "0.1", "--epochs", "1", "--log_dir", "9152"], c["env"])
    c["run"](c["base"] + ["--epochs", "1", "--log_dir", "9153"], c["env"])
    first = _ckpt(c["out_dir"], 9151, 0)
    assert _equal_ckpt(first, _ckpt(c["out_dir"], 9152, 0))
    assert not _equal_ckpt(first, _ckpt(c["out_dir"], 9153, 0))
    sd = torch.load(first, map_location="cpu")
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())


def test_cli_stage1_dropout_resumes_bit_exactly(cli_tree):
    """One epoch plus --resume equals two epochs, bit for bit (the train state carries the dropout counter)."""
    c = cli_tree
    args = c["base"] + ["--imu_dropout", "0.1", "--epochs", "2"]
    c["run"](args + ["--log_dir", "9154"], c["env"])
    out = c["run"](args + ["--log_dir", "9155", "--resume", _ckpt(c["out_dir"], 9151, 0)], c["env"])
    assert "resumed from" in out and "epoch: 2" in out and "epoch: 1\n" not in out
    a, b = _ckpt(c["out_dir"], 9154, 1), _ckpt(c["out_dir"], 9155, 1)
    assert _equal_ckpt(a, b)
    ta = torch.load(a[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)
    tb = torch.load(b[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)
    assert torch.equal(ta["dropout_counter"], tb["dropout_counter"]) and torch.equal(ta["optimizer"]["m"], tb["optimizer"]["m"])
    t0 = torch.load(_ckpt(c["out_dir"], 9151, 0)[:-4] + ".train_state.pth", map_location="cpu", weights_only=False)
    assert not torch.equal(t0["dropout_counter"], ta["dropout_counter"])
    assert _word(t0["dropout_counter"]) != DEFAULT_WORD                          # (the counter really moves under the flag)


def test_cli_finetune_with_dropout(cli_tree):
    """--train --network Upper_Net --finetune_imu --imu_dropout 0.1 --epochs 1 --seed 0: both checkpoints, finite losses, the IMU_Net's
    weights moved."""
    from mmego_amd import nets
    c = cli_tree
    torch.manual_seed(2)
    imu_ck = str(c["tmp"] / "imu.pth")
    start = {k: v.clone() for k, v in nets.IMUNet(15, 9, 512, 2, True, 0.1).state_dict().items()}
    torch.save(start, imu_ck)
    out = c["run"](["--train", "--network", "Upper_Net", "--load_IMU_path", imu_ck, "--data_root", c["data"], "--epochs", "1",
                    "--batch_size", "3", "--device", "cuda:0", "--seed", "0", "--finetune_imu", "--imu_dropout", "0.1", "--log_dir", "9156"],
                   c["env"])
    assert "epoch: 1" in out and "Average Joint Localization Error" in out
    mdir = os.path.join(c["out_dir"], "model", "9156")
    up = _ckpt(c["out_dir"], 9156, 0)
    im = glob.glob(os.path.join(mdir, "IMU_Net", "epoch0_batch3frame*.pth"))
    assert len(im) == 1 and os.path.basename(up) == os.path.basename(im[0])
    nets.UpperNet().load_state_dict(torch.load(up, map_location="cpu"))
    got = torch.load(im[0], map_location="cpu")
    assert got.keys() == start.keys()
    for k in start:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], start[k]) == k.startswith("fc3."), k
    log = open(os.path.join(c["out_dir"], "report", "9156", "log-loss.txt")).read().split()
    assert np.isfinite(float(log[1]))
