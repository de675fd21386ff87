"""GPU: the 4-row form of the H = 64 BiLSTM recurrence kernels (csrc/lstm.hip, ROWS = 4: v_mfma_f32_4x4x1_16B_f32, one cell per lane) --
what mmego_lstm64_forward / _backward and their _multi forms take while the 16-row grid covers at most half of the chip.

The reference is a float64 LSTM cell recurrence written out below (PyTorch gate order i, f, g, o; both directions; the backward on the
stashes it is given), from the fp32 values the kernels read.  The error bar is not a number chosen here: the 16-row form (forced through
the launcher by MMEGO_LSTM64_ROWS=16) runs on the SAME inputs against the SAME reference (fixture `bar`), and in every case, for every
output, the 4-row form's largest |out - ref| may be at most twice the 16-row form's.  Beyond that bar: the 4-row kernels add the terms
of a product on ONE accumulator in the order in which the 16-row form's v_mfma_f32_16x16x4_f32 chains take them, so every output of
every case has the 16-row form's BITS, which is asserted as well (the bar then holds with equality; it stays, should the order ever
change).  The a-priori bounds of tests/lstm_ref.py are held by tests/test_lstm_kernels_gpu.py, whose batch sizes take the 4-row form as
well.  NOTES.md "BiLSTM(64) recurrences: four-row workgroups" records the figures.

Buffers are test_lstm_kernels_gpu.py's: strided operands in wider buffers with NaN around them, every output surrounded by a sentinel
that must survive -- B = 1 and B = 5 leave three lanes of the last workgroup's every quad without a row."""
import contextlib
import os

import numpy as np
import pytest
import torch

import lstm_ref as R
import pose_noise_ref as PN
from test_gcn_train_gpu import call
from test_lstm_kernels_gpu import L64, L64B, DROP_P, same_bits

pytestmark = pytest.mark.gpu

ENV = "MMEGO_LSTM64_ROWS"
L4_B = (1, 4, 5, 64)
L4_T = (1, 2, 8)
FIGURES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mmego_amd import hip
    hip.lib()
    assert ENV not in os.environ, "%s is set: the dispatch under test is the launchers' own" % ENV
    yield torch.device("cuda:0")
    if FIGURES:
        print("\nlargest |out - ref| against float64 over all cases, per output: 4-row form, 16-row form")
        for k, (e4, e16) in sorted(FIGURES.items()):
            print("ROWS4 %-22s %.4g %.4g" % (k, e4, e16))


@contextlib.contextmanager
def forced_rows(rows):
    """The launchers read the variable per call."""
    os.environ[ENV] = str(rows)
    try:
        yield
    finally:
        del os.environ[ENV]


def rows_at(B):
    from mmego_amd import hip
    return hip.lib().mmego_lstm64_rows(B)


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def ref_forward(I, o, B, T):
    """-> out [B][T][128], hn / cn [2][B][64], gates[d] [T][B][64][4] (i, f, g, o), cst[d] [T][B][64], hprev[d] [B][T][64]."""
    r = {"out": torch.zeros(B, T, 128, dtype=torch.float64), "hn": [], "cn": [], "gates": [], "cst": [], "hprev": []}
    for d in range(2):
        W, b = I["W"][d].double(), (I["b"][d].double() if I["b"][d] is not None else torch.zeros(256, dtype=torch.float64))
        h = I["h0"][d].double() if o["h0"][d] else torch.zeros(B, 64, dtype=torch.float64)
        c = I["c0"][d].double() if o["c0"][d] else torch.zeros(B, 64, dtype=torch.float64)
        gates, cst, hprev = torch.zeros(T, B, 64, 4, dtype=torch.float64), torch.zeros(T, B, 64, dtype=torch.float64), torch.zeros(B, T, 64, dtype=torch.float64)
        for s in range(T):
            t = s if d == 0 else T - 1 - s
            hprev[:, t] = h
            P = I["xp"][d][:, t].double() + b + h @ W.t()
            gi, gf, gg, go = torch.sigmoid(P[:, 0:64]), torch.sigmoid(P[:, 64:128]), torch.tanh(P[:, 128:192]), torch.sigmoid(P[:, 192:256])
            c = gf * c + gi * gg
            h = go * torch.tanh(c)
            gates[t], cst[t] = torch.stack((gi, gf, gg, go), -1), c
            r["out"][:, t, d * 64:(d + 1) * 64] = h
        r["hn"].append(h); r["cn"].append(c); r["gates"].append(gates); r["cst"].append(cst); r["hprev"].append(hprev)
    return r


def ref_backward(I, o, gates, cst, B, T):
    """dgates[d] [B][T][256] (gate-major columns) from the fp32 stashes the kernel reads."""
    res = []
    for d in range(2):
        W, G, C = I["W"][d].double(), gates[d].double(), cst[d].double()
        dg = torch.zeros(B, T, 256, dtype=torch.float64)
        dc, rec = torch.zeros(B, 64, dtype=torch.float64), torch.zeros(B, 64, dtype=torch.float64)
        for s in range(T - 1, -1, -1):
            t = s if d == 0 else T - 1 - s
            tp = t - 1 if d == 0 else t + 1
            cprev = C[tp] if s > 0 else (I["c0"][d].double() if o["bc0"][d] else torch.zeros(B, 64, dtype=torch.float64))
            gi, gf, gg, go = G[t, :, :, 0], G[t, :, :, 1], G[t, :, :, 2], G[t, :, :, 3]
            dh = I["dout"][:, t, d * 64:(d + 1) * 64].double() + rec
            tc = torch.tanh(C[t])
            dcv = dc + dh * go * (1 - tc * tc)
            dg[:, t] = torch.cat((dcv * gg * gi * (1 - gi), dcv * cprev * gf * (1 - gf), dcv * gi * (1 - gg * gg), dh * tc * go * (1 - go)), -1)
            dc = dcv * gf
            rec = dg[:, t] @ W
        res.append(dg)
    return res


def host_mask(B, T, os_, seed, salt, p):
    """drop_mask [B][T][128] as csrc/common.h's dropout_keep gives it: element index = the offset into out's buffer (row stride os)."""
    key = PN.dropout_key(seed, salt)
    idx = (np.arange(B * T, dtype=np.uint64)[:, None] * np.uint64(os_) + np.arange(128, dtype=np.uint64)[None, :]) & np.uint64(PN.M32)
    u = (PN.hash32(idx ^ np.uint64(key)) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    keep = u >= np.float32(p)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return torch.from_numpy(np.where(keep, scale, np.float32(0.0)).astype(np.float32)).view(B, T, 128)


def worst(got, ref):
    return float((got.double() - ref).abs().max())


def errors(g, ref, stash):
    """largest |out - ref| per output (both directions together)."""
    e = {"out": worst(g["out"], ref["out"]), "hn": max(worst(g["hn"][d], ref["hn"][d]) for d in range(2)),
         "cn": max(worst(g["cn"][d], ref["cn"][d]) for d in range(2))}
    if stash:
        for k in ("gates", "cst", "hprev"):
            e[k] = max(worst(g[k][d], ref[k][d]) for d in range(2))
    return e


def hold(bar, kernel, e4, note):
    """Every figure printed before anything is asserted: this case's 4-row and 16-row errors."""
    e16 = bar["case"][(kernel, note)]
    for k in e4:
        print("rows4 %s %s %s: 4-row %.4g, 16-row %.4g" % (kernel, note, k, e4[k], e16[k]))
        f = FIGURES.get(kernel + " " + k, (0.0, 0.0))
        FIGURES[kernel + " " + k] = (max(f[0], e4[k]), max(f[1], e16[k]))
    for k in e4:
        assert e4[k] <= 2.0 * e16[k], (kernel, k, "4-row %.6g > 2 x 16-row %.6g" % (e4[k], e16[k]), note)


def same_outputs(a, b):
    """Every output of two runs bit for bit -> the names that differ."""
    return [k for k in a for x, y in zip(a[k] if isinstance(a[k], list) else [a[k]], b[k] if isinstance(b[k], list) else [b[k]]) if not same_bits(x, y)]


_CASES = {}


def fwd_case(B, T, oi):
    """Inputs and float64 forward of a case, computed once."""
    if ("f", B, T, oi) not in _CASES:
        I = R.seq_inputs(B, T, oi, with_b=R.L64_OPTS[oi]["bhh"])
        _CASES[("f", B, T, oi)] = (I, ref_forward(I, R.L64_OPTS[oi], B, T))
    return _CASES[("f", B, T, oi)]


def bwd_case(B, T, oi):
    """Inputs, fp32 stashes (the float64 forward's, rounded: the same for both forms, and a forward error cannot hide a backward one) and
    float64 backward of a case, computed once."""
    if ("b", B, T, oi) not in _CASES:
        o = R.L64_OPTS[oi]
        I = R.seq_inputs(B, T, oi, with_b=o["bhh"])
        f = ref_forward(I, dict(o, c0=o["bc0"]), B, T)
        gates, cst = [g.float() for g in f["gates"]], [c.float() for c in f["cst"]]
        _CASES[("b", B, T, oi)] = (I, gates, cst, ref_backward(I, o, gates, cst, B, T))
    return _CASES[("b", B, T, oi)]


def bwd_error(got, ref):
    return {"dgates": max(worst(got[d], ref[d]) for d in range(2))}


@pytest.fixture(scope="module")
def bar(dev):
    """The 16-row form on every case of the file, run once: its largest error per case and output (the bar) and its outputs."""
    b = {"case": {}, "out": {}}

    def note_down(kernel, note, e, outputs):
        b["case"][(kernel, note)], b["out"][(kernel, note)] = e, outputs

    with forced_rows(16):
        for B in L4_B:
            for T in L4_T:
                for oi, o in enumerate(R.L64_OPTS):
                    I, ref = fwd_case(B, T, oi)
                    for stash in (0, 1):
                        for drop in (0, 1):
                            g16 = L64(dev, I, B, T, o, stash, drop).run().outputs()
                            note_down("lstm64_fwd", (B, T, oi, stash, drop), errors(g16, ref, stash), g16)
                    I, gates, cst, ref = bwd_case(B, T, oi)
                    got16 = L64B(dev, I, B, T, o, gates, cst).run().result()
                    note_down("lstm64_bwd", (B, T, oi), bwd_error(got16, ref), {"dgates": got16})
    return b


# ---------------------------------------------------------------------------------------------------------------------------------
# forward and backward against float64, the 16-row form's error as the bar
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", L4_T)
@pytest.mark.parametrize("B", L4_B)
def test_rows4_forward(dev, bar, B, T):
    """Both directions; stashes and dropout on and off; h0 / c0 given for both directions, one each, or none (R.L64_OPTS: strides 512 / 516
    and 128 / 256 as well); the mask against dropout_keep on the host."""
    assert rows_at(B) == 4
    for oi, o in enumerate(R.L64_OPTS):
        I, ref = fwd_case(B, T, oi)
        plain = {}
        for stash in (0, 1):
            for drop in (0, 1):
                note = (B, T, oi, stash, drop)
                run = L64(dev, I, B, T, o, stash, drop).run()
                g = run.outputs()
                assert run.guards(), ("guards", note)
                hold(bar, "lstm64_fwd", errors(g, ref, stash), note)
                assert same_outputs(g, bar["out"][("lstm64_fwd", note)]) == [], ("not the 16-row form's bits", note)
                if stash:
                    for d in range(2):
                        order = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
                        own = torch.stack([g["out"][:, order[s - 1], d * 64:(d + 1) * 64] if s > 0 else
                                           (I["h0"][d] if o["h0"][d] else torch.zeros(B, 64)) for s in range(T)], 1)
                        assert same_bits(g["hprev"][d][:, order], own), ("hprev is not the kernel's own h_{t-1}", note)
                        assert same_bits(g["hn"][d], g["out"][:, order[-1], d * 64:(d + 1) * 64]) and same_bits(g["cn"][d], g["cst"][d][order[-1]]), note
                if drop:
                    assert same_bits(g["dm"], host_mask(B, T, o["os"], 12345, run.salt, DROP_P)), ("drop_mask is not dropout_keep's", note)
                    assert same_bits(g["dy"], g["out"] * g["dm"]), note
                    assert same_bits(g["out"], plain[stash]["out"]), ("out with and without dropout", note)
                else:
                    plain[stash] = g


@pytest.mark.parametrize("T", L4_T)
@pytest.mark.parametrize("B", L4_B)
def test_rows4_backward(dev, bar, B, T):
    """Stashes: the float64 forward's, rounded to fp32 (bwd_case); c0 given for both directions, one each, or none."""
    assert rows_at(B) == 4
    for oi, o in enumerate(R.L64_OPTS):
        I, gates, cst, ref = bwd_case(B, T, oi)
        run = L64B(dev, I, B, T, o, gates, cst).run()
        got = run.result()
        assert run.dg.guards_intact() and run.dout.guards_intact(), ("guards", B, T, oi)
        hold(bar, "lstm64_bwd", bwd_error(got, ref), (B, T, oi))
        assert same_outputs({"dgates": got}, bar["out"][("lstm64_bwd", (B, T, oi))]) == [], ("not the 16-row form's bits", B, T, oi)


def test_rows4_backward_from_kernel_stashes(dev, bar):
    """The workload's shape with the stashes the 4-row forward wrote (what a training step does); the 16-row backward on the same
    stashes beside it."""
    B, T, o = 64, 8, R.L64_OPTS[0]
    I = R.seq_inputs(B, T, 7)
    f = L64(dev, I, B, T, dict(o, c0=o["bc0"]), 1, 0).run().outputs()
    ref = ref_backward(I, o, f["gates"], f["cst"], B, T)
    got = L64B(dev, I, B, T, o, f["gates"], f["cst"]).run().result()
    with forced_rows(16):
        got16 = L64B(dev, I, B, T, o, f["gates"], f["cst"]).run().result()
    bar["case"][("lstm64_bwd", (B, T, "kernel stashes"))] = bwd_error(got16, ref)
    hold(bar, "lstm64_bwd", bwd_error(got, ref), (B, T, "kernel stashes"))
    assert same_outputs({"dgates": got}, {"dgates": got16}) == []


# ---------------------------------------------------------------------------------------------------------------------------------
# two stacks in one launch, and which form a batch size takes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rows4_two_stacks_are_the_single_launches(dev):
    """B = 64, T = 8: mmego_lstm64_forward_multi / _backward_multi with two stacks give the bits of the single-stack launches -- the same
    body with the same ROWS (the form is a function of B alone, not of the number of stacks)."""
    from mmego_amd import hip
    B, T, n = 64, 8, 2
    assert rows_at(B) == 4
    Is = [R.seq_inputs(B, T, 20 + i, with_b=R.L64_OPTS[i]["bhh"]) for i in range(n)]
    for stash, drop in ((1, 1), (0, 0)):
        single = [L64(dev, Is[i], B, T, R.L64_OPTS[i], stash, drop, salt=i).run() for i in range(n)]
        multi = [L64(dev, Is[i], B, T, R.L64_OPTS[i], stash, drop, salt=i) for i in range(n)]
        call("lstm64_forward_multi", n, (hip.Lstm64Fwd * n)(*[m.desc() for m in multi]))
        for i in range(n):
            a, b = single[i].outputs(), multi[i].outputs()
            assert multi[i].guards(), i
            for key in a:
                for x, y in zip(a[key] if isinstance(a[key], list) else [a[key]], b[key] if isinstance(b[key], list) else [b[key]]):
                    assert same_bits(x, y), (i, key, stash, drop)
    f = [L64(dev, Is[i], B, T, dict(R.L64_OPTS[i], c0=R.L64_OPTS[i]["bc0"]), 1, 0).run().outputs() for i in range(n)]
    sb = [L64B(dev, Is[i], B, T, R.L64_OPTS[i], f[i]["gates"], f[i]["cst"]).run() for i in range(n)]
    mb = [L64B(dev, Is[i], B, T, R.L64_OPTS[i], f[i]["gates"], f[i]["cst"]) for i in range(n)]
    call("lstm64_backward_multi", n, (hip.Lstm64Bwd * n)(*[m.desc() for m in mb]))
    for i in range(n):
        assert mb[i].dg.guards_intact() and same_bits(sb[i].dg.view, mb[i].dg.view), i


def both_passes(dev, I, B, T, o):
    """Forward with stashes and dropout, backward on its stashes: every output of the two calls."""
    f = L64(dev, I, B, T, dict(o, c0=o["bc0"]), 1, 1).run().outputs()
    f["dgates"] = L64B(dev, I, B, T, o, f["gates"], f["cst"]).run().result()
    return f


def all_same_bits(a, b):
    return all(same_bits(x, y) for k in a for x, y in zip(a[k] if isinstance(a[k], list) else [a[k]], b[k] if isinstance(b[k], list) else [b[k]]))


def test_rows4_dispatch(dev):
    """B = 64 (8 workgroups of 16 rows on the whole chip) takes ROWS = 4; the first B whose 16-row grid covers more than half of the CUs
    takes ROWS = 16 and gives the bits of the 16-row instantiation forced through the launcher, the B one row below it ROWS = 4.  The
    choice depends on B alone, so the calls of one shape agree with each other."""
    o, T = R.L64_OPTS[2], 2
    I = R.seq_inputs(64, T, 30)
    auto = both_passes(dev, I, 64, T, o)
    with forced_rows(4):
        f4 = both_passes(dev, I, 64, T, o)
    with forced_rows(16):
        f16 = both_passes(dev, I, 64, T, o)
    assert rows_at(64) == 4 and all_same_bits(auto, f4)
    assert all_same_bits(f4, f16)           # (the two forms add in the same order: which one ran is told by mmego_lstm64_rows alone)
    big = 16 * (cu_count() // 4) + 1                     # 2 * ceil(big / 16) * 2 > CUs
    assert rows_at(big) == 16 and rows_at(big - 1) == 4 and rows_at(big + 16) == 16 and rows_at(2 * big) == 16
    I = R.seq_inputs(big, T, 31)
    auto = both_passes(dev, I, big, T, o)
    with forced_rows(16):
        f16 = both_passes(dev, I, big, T, o)
    assert all_same_bits(auto, f16)
    with forced_rows(16):
        assert rows_at(64) == 16
    with forced_rows(4):
        assert rows_at(2 * big) == 4
