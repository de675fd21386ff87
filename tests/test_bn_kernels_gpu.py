"""GPU: the kernels of csrc/bn.hip, each entry point on its own through the C ABI, against float64 (tests/bn_ref.py): the train-mode
BatchNorm statistics and running-stat updates (single, pair, finalize alone on hand-made records), the eval fold (bn_eval_affine,
bn_fold_linear), the affine + ReLU pass, the BatchNorm backward (single, pair), a forward-backward chain against float64 autograd, the
column sums on every path (short, 16-row blocks, 16-byte loads; pair; colsum2) and the bit-exact helpers copy2d, copy2d_pair, relu_mask
and fill.

Method of tests/test_pool_kernels_gpu.py, tests/test_gcn_train_gpu.py and tests/test_lstm_kernels_gpu.py (their helpers are used): every
reference is plain float64 torch on the CPU computed from the fp32 values the kernel read; |out - ref| <= MARGIN * bound elementwise with
the a-priori bounds bn_ref.py derives (MARGIN = 4); no element is left out; every operand lies inside a wider NaN-filled buffer with a row
stride of its own, different from C and from its neighbours'; every output, workspaces included, sits between sentinels that must survive;
every case runs twice and the two runs have the same bits.  Every statistics, backward and column-sum tensor mixes six kinds of column:
randn, 1000 + 0.01 randn, constant, the first row of every block an outlier of 1e4, one nonzero among zeros, and +-1e4 alternating plus
noise.  Bits are asked where a result is ONE rounding of values the test can see (the device code is compiled with contraction allowed):
b, a from the kernel's own invstd, running statistics under momentum 0 and 1, the scaled and the accumulated column sums from an unscaled
call, the pair forms from the single ones, the copies.  NOTES.md ("Float64 tests of bn.hip") holds the measured error / bound ratios;
tests/test_bn_ref_cpu.py pins which kernel and branch each case reaches."""
import ctypes
import struct

import pytest
import torch
import torch.nn.functional as F

import bn_ref as R
import test_lstm_kernels_gpu as L
from bn_ref import MARGIN, D
from test_lstm_kernels_gpu import Wide, same_bits
from test_gcn_train_gpu import Out, d_vec, d_mat, refused, call, NAN  # noqa: F401  (the shared helpers of the kernel test files)

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mmego_amd import hip
    hip.lib()
    yield torch.device("cuda:0")
    if RATIOS:
        print("\nlargest |out - ref| / bound per kernel and output (bound without MARGIN):")
        for (k, o), r in sorted(RATIOS.items()):
            print("RATIO %-26s %-16s %.4g" % (k, o, r))


def check(kernel, name, out, ref, bound, note=""):
    """test_lstm_kernels_gpu.check, with the ratio kept in this file's table (as tests/test_pool_kernels_gpu.py does; the kernel names
    used here -- bn_*, affine_act, colsum*, chain* -- are none of the LSTM file's)."""
    try:
        L.check(kernel, name, out, ref, bound, note)
    finally:
        RATIOS[(kernel, name)] = max(RATIOS.get((kernel, name), 0.0), L.RATIOS.pop((kernel, name), 0.0))


def operand(dev, T, extra, col=1, lead=0):
    """T [rows][C] at column `col` of a NaN-filled buffer of row stride C + extra."""
    rows, C = T.shape
    return Wide(dev, rows, C, C + extra, col=col, fill=NAN, src=T, lead=lead)


def vec_out(dev, n, init=None):
    """n floats with the sentinel in front of and behind them."""
    w = Wide(dev, 1, n, n + 8, col=4)
    if init is not None:
        w.view.copy_(init.view(1, -1))
    return w


def result(w):
    return w.cpu().reshape(-1)


def twice(run):
    """Nothing depends on scheduling: two runs, the same bits."""
    a, b = run(), run()
    assert a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a), "two launches differ"
    return a


def intact(*bufs):
    return all(b.guards_intact() for b in bufs if b is not None)


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_bn_train_stats, _pair, mmego_bn_finalize
# ---------------------------------------------------------------------------------------------------------------------------------
STATE = ("mean", "invstd", "a", "b")


def run_stats(dev, X, p, extra=3):
    rows, C = X.shape
    g, b, rm, rv, mom, eps = p
    Xw = operand(dev, X, extra)
    ws = vec_out(dev, 3 * C * R.nblk(rows))
    outs = {k: vec_out(dev, C) for k in STATE}
    if rm is not None:
        outs["running_mean"], outs["running_var"] = vec_out(dev, C, rm), vec_out(dev, C, rv)
    call("bn_train_stats", Xw.view, Xw.ld, rows, C, d_vec(dev, g), d_vec(dev, b), outs["running_mean"].view if rm is not None else None,
         outs["running_var"].view if rm is not None else None, mom, eps, ws.view, *[outs[k].view for k in STATE])
    assert intact(Xw, ws, *outs.values()), ("guards", rows, C)
    return {k: result(v) for k, v in outs.items()}


def check_state(kernel, got, ref, p, note):
    """Against float64, and the bits a single rounding fixes."""
    g, b, rm, rv, mom, eps = p
    assert set(got) == set(ref)
    for k in ref:
        check(kernel, k, got[k], *ref[k], note)
    assert same_bits(got["b"], b), ("b has the bits of beta", note)
    assert same_bits(got["a"], g * got["invstd"]), ("a is one product of gamma and the stored invstd", note)
    if rm is not None and mom == 0.0:
        assert same_bits(got["running_mean"], rm) and same_bits(got["running_var"], rv), ("momentum 0 leaves the running statistics alone", note)
    if rm is not None and mom == 1.0:
        assert torch.equal(got["running_mean"], got["mean"]), ("momentum 1: running_mean is mean", note)


@pytest.mark.parametrize("case", R.STATS_CASES, ids=lambda c: "%d-%d" % c[:2])
def test_bn_train_stats(dev, case):
    X, kinds, p = R.stats_inputs(case)
    got = twice(lambda: run_stats(dev, X, p))
    check_state("bn_train_stats", got, R.train_stats(X, *p), p, case)
    const = kinds == 2
    assert bool((got["invstd"][const] == (1.0 / torch.sqrt(R.f32(case[4]).double())).float()).all()), ("a constant column has variance exactly 0", case)
    assert bool((got["mean"][const] == R.f32(R.CONST)).all())


@pytest.mark.parametrize("nb", R.FINALIZE_NBLK)
def test_bn_finalize_on_hand_made_records(dev, nb):
    """Records [C][nb][3] with NaN behind them (a lane k >= nb reads the clamped record 0 and discards it); with running statistics and
    with both NULL."""
    C = 5
    n, m, q = R.hand_records(nb, C, 1)
    g, b, rm, rv = R.bn_params(C, 12)
    rec = torch.full((C * nb * 3 + 192,), NAN)
    rec[:C * nb * 3] = torch.stack((n, m, q), -1).permute(1, 0, 2).reshape(-1)
    rec = rec.to(dev)
    for run_given in (True, False):
        p = (g, b, rm if run_given else None, rv if run_given else None, 0.1, 1e-5)

        def run():
            outs = {k: vec_out(dev, C) for k in STATE}
            if run_given:
                outs["running_mean"], outs["running_var"] = vec_out(dev, C, rm), vec_out(dev, C, rv)
            call("bn_finalize", rec, nb, C, d_vec(dev, g), d_vec(dev, b), outs["running_mean"].view if run_given else None,
                 outs["running_var"].view if run_given else None, 0.1, 1e-5, *[outs[k].view for k in STATE])
            assert intact(*outs.values())
            return {k: result(v) for k, v in outs.items()}
        check_state("bn_finalize", twice(run), R.finalize(n, m, q, *p), p, (nb, run_given))


@pytest.mark.parametrize("case", R.PAIR_CASES, ids=lambda c: "%d-%d" % c)
def test_bn_train_stats_pair(dev, case):
    """Two BatchNorms of different gamma, beta, momentum and eps, one of them without running statistics (which one alternates): each
    against float64, and the bits of two mmego_bn_train_stats calls."""
    rows, C = case
    X1, X2 = R.columns(rows, C, 21)[0], R.columns(rows, C, 22, first=3)[0]
    first_null = bool(rows & 1)
    q1, q2 = R.bn_params(C, 21), R.bn_params(C, 22)
    p1 = (q1[0], q1[1]) + ((None, None) if first_null else q1[2:]) + (0.1, 1e-5)
    p2 = (q2[0], q2[1]) + (q2[2:] if first_null else (None, None)) + (0.3, 1e-3)

    def run():
        Xw = [operand(dev, X1, 3), operand(dev, X2, 6, col=2)]
        ws = vec_out(dev, 6 * C * R.nblk(rows))
        outs, args = {}, []
        for i, (Xi, p) in enumerate(zip(Xw, (p1, p2))):
            o = {k: vec_out(dev, C) for k in STATE}
            if p[2] is not None:
                o["running_mean"], o["running_var"] = vec_out(dev, C, p[2]), vec_out(dev, C, p[3])
            args += [Xi.view, Xi.ld, d_vec(dev, p[0]), d_vec(dev, p[1]), o["running_mean"].view if p[2] is not None else None,
                     o["running_var"].view if p[2] is not None else None, p[4], p[5]] + [o[k].view for k in STATE]
            outs.update({"%s%d" % (k, i + 1): v for k, v in o.items()})
        call("bn_train_stats_pair", rows, C, ws.view, *args)
        assert intact(ws, *Xw, *outs.values()), ("guards", case)
        return {k: result(v) for k, v in outs.items()}
    got = twice(run)
    for i, (X, p) in enumerate(((X1, p1), (X2, p2))):
        mine = {k[:-1]: v for k, v in got.items() if k.endswith(str(i + 1))}
        check_state("bn_train_stats_pair", mine, R.train_stats(X, *p), p, case + (i + 1,))
        single = run_stats(dev, X, p, 5)
        assert all(same_bits(mine[k], single[k]) for k in single), ("the pair has the bits of two single calls", case, i + 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_bn_eval_affine, mmego_bn_fold_linear
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.EVAL_C)
def test_bn_eval_affine(dev, C):
    g, b, rm, rv = R.bn_params(C, 31)
    rv[C // 2] = 0.0
    for eps in (1e-5, 1e-3):
        def run():
            outs = {k: vec_out(dev, C) for k in STATE}
            call("bn_eval_affine", C, d_vec(dev, g), d_vec(dev, b), d_vec(dev, rm), d_vec(dev, rv), eps, *[outs[k].view for k in STATE])
            assert intact(*outs.values())
            return {k: result(v) for k, v in outs.items()}
        got, ref = twice(run), R.eval_affine(g, b, rm, rv, eps)
        for k in ref:
            check("bn_eval_affine", k, got[k], *ref[k], (C, eps))
        assert same_bits(got["mean"], rm) and same_bits(got["b"], b) and same_bits(got["a"], g * got["invstd"]), (C, eps)


@pytest.mark.parametrize("bias", (True, False))
@pytest.mark.parametrize("case", R.FOLD_CASES, ids=lambda c: "%d-%d" % c)
def test_bn_fold_linear(dev, case, bias):
    N, K = case
    gen = R.gen_for(N, K, 33)
    W, b, x = torch.randn(N, K, generator=gen), torch.randn(N, generator=gen) if bias else None, torch.randn(8, K, generator=gen)
    g, be, rm, rv = R.bn_params(N, 33)
    rv[N // 2] = 0.0

    def run():
        Wf, bf = Out(dev, N, K, strided=False), vec_out(dev, N)
        call("bn_fold_linear", d_vec(dev, W), None if b is None else d_vec(dev, b), N, K, d_vec(dev, g), d_vec(dev, be), d_vec(dev, rm),
             d_vec(dev, rv), 1e-5, Wf.view, bf.view)
        assert intact(Wf, bf)
        return {"Wf": Wf.cpu(), "bf": result(bf)}
    got, ref = twice(run), R.fold_linear(W, b, g, be, rm, rv, 1e-5)
    check("bn_fold_linear", "Wf", got["Wf"], *ref["Wf"], case)
    check("bn_fold_linear", "bf", got["bf"], *ref["bf"], case)
    # the folded layer is BatchNorm(eval) behind the layer: float64 from the kernel's fp32 Wf / bf, the bounds carried through the product
    pre = D(x) @ D(W).t() + (0.0 if b is None else D(b))
    want = F.batch_norm(pre, D(rm), D(rv), D(g), D(be), False, 0.0, float(R.f32(1e-5)))
    check("bn_fold_linear", "x Wf^T + bf", D(x) @ D(got["Wf"]).t() + D(got["bf"]), want, D(x).abs() @ ref["Wf"][1].t() + ref["bf"][1], case)


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_affine_act
# ---------------------------------------------------------------------------------------------------------------------------------
def run_affine(dev, relu, X1, s1, X2=None, s2=None):
    """s = (mean, a, b) -> Y on the CPU; the three tensors have three different strides."""
    rows, C = X1.shape
    w1, w2 = operand(dev, X1, 3), None if X2 is None else operand(dev, X2, 5, col=2)
    Y = Wide(dev, rows, C, C + 2, col=1)
    v1 = [d_vec(dev, t) for t in s1]
    v2 = [None] * 3 if X2 is None else [d_vec(dev, t) for t in s2]
    call("affine_act", w1.view, w1.ld, *v1, None if X2 is None else w2.view, 0 if X2 is None else w2.ld, *v2, Y.view, Y.ld, rows, C, relu)
    assert intact(w1, w2, Y), ("guards", rows, C)
    return Y.cpu()


def affine_state(C, key):
    mean, _, a = R.given_state(C, key)
    return mean, a, torch.randn(C, generator=R.gen_for(C, key, 3)) * 0.3


@pytest.mark.parametrize("case", R.AFFINE_CASES, ids=lambda c: "%d-%d" % c)
def test_affine_act(dev, case):
    rows, C = case
    X1, X2 = R.columns(rows, C, 35)[0], torch.randn(rows, C, generator=R.gen_for(rows, C, 36))
    s1, s2 = affine_state(C, 35), affine_state(C, 36)
    for two in (False, True):
        args = (X1, *s1) + ((X2, *s2) if two else ())
        pre, e = R.affine_pre(*args)
        for relu in (0, 1):
            got = twice(lambda: {"Y": run_affine(dev, relu, X1, s1, X2 if two else None, s2)})["Y"]
            check("affine_act", "Y%s%s" % (" two" if two else "", " relu" if relu else ""), got, *R.affine_act(relu, *args), (case, two, relu))
            if relu:
                assert bool((got >= 0).all()), ("no output of a ReLU is negative", case, two)
                assert bool((got[pre < -e] == 0).all()), ("0 where the pre-activation lies below minus its bound", case, two)
                assert rows * C < 100 or bool((pre < -e).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_bn_backward, _pair
# ---------------------------------------------------------------------------------------------------------------------------------
def run_backward(dev, dY, M, Xs, states):
    """One BatchNorm (mmego_bn_backward) or two that share dY and the mask (_pair); states: (mean, invstd, a) each.
    -> {"dgamma1", "dbeta1", "dX1", ..}"""
    rows, C = dY.shape
    n = len(Xs)
    dYw, Mw = operand(dev, dY, 1, col=0), None if M is None else operand(dev, M, 2)
    ws, c12 = vec_out(dev, 2 * n * C * R.nblk(rows)), vec_out(dev, 2 * n * C)
    outs, per = {}, []
    for i, (X, st) in enumerate(zip(Xs, states)):
        Xw, dX = operand(dev, X, 3 + 4 * i, col=2), Wide(dev, rows, C, C + 5 + i, col=2)
        dg, db = vec_out(dev, C), vec_out(dev, C)
        outs.update({"dgamma%d" % (i + 1): dg, "dbeta%d" % (i + 1): db, "dX%d" % (i + 1): dX})
        per.append([Xw.view, Xw.ld] + [d_vec(dev, t) for t in st] + [dg.view, db.view, dX.view, dX.ld])
        outs["_X%d" % i] = Xw
    mask = (None, 0) if M is None else (Mw.view, Mw.ld)
    if n == 1:
        x = per[0]
        call("bn_backward", dYw.view, dYw.ld, *mask, x[0], x[1], x[2], x[3], x[4], rows, C, ws.view, c12.view, x[5], x[6], x[7], x[8])
    else:
        call("bn_backward_pair", dYw.view, dYw.ld, *mask, rows, C, ws.view, c12.view, *per[0], *per[1])
    assert intact(dYw, Mw, ws, c12, *outs.values()), ("guards", rows, C)
    return {k: (v.cpu() if k.startswith("dX") else result(v)) for k, v in outs.items() if not k.startswith("_")}


@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: "%d-%d-%d" % c)
def test_bn_backward(dev, case):
    """mean, invstd and a are NOT the batch's own: the kernel is a formula of the state it is handed.  The mask holds positives,
    negatives, +0, -0, denormals of both signs and NaN; only `mask > 0` passes."""
    rows, C, masked = case
    X, _ = R.columns(rows, C, 13)
    dY, M = torch.randn(rows, C, generator=R.gen_for(rows, C, 14)), R.mask_values(rows, C, 13) if masked else None
    st = R.given_state(C, 13)
    got, ref = twice(lambda: run_backward(dev, dY, M, [X], [st])), R.bn_backward(dY, M, X, *st)
    for k in ("dgamma", "dbeta", "dX"):
        check("bn_backward", k, got[k + "1"], *ref[k], case)


@pytest.mark.parametrize("case", R.BWD_PAIR_CASES, ids=lambda c: "%d-%d" % c)
def test_bn_backward_pair(dev, case):
    rows, C = case
    X1, X2 = R.columns(rows, C, 15)[0], R.columns(rows, C, 16, first=2)[0]
    dY, M = torch.randn(rows, C, generator=R.gen_for(rows, C, 17)), R.mask_values(rows, C, 15)
    s1, s2 = R.given_state(C, 15), R.given_state(C, 16)
    got = twice(lambda: run_backward(dev, dY, M, [X1, X2], [s1, s2]))
    for i, (X, st) in enumerate(((X1, s1), (X2, s2))):
        ref = R.bn_backward(dY, M, X, *st)
        for k in ("dgamma", "dbeta", "dX"):
            check("bn_backward_pair", "%s%d" % (k, i + 1), got["%s%d" % (k, i + 1)], *ref[k], case)


# ---------------------------------------------------------------------------------------------------------------------------------
# chain: statistics -> affine + ReLU -> backward, against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------------------
def check_chain(dev, rows, C, n):
    """n BatchNorms summed behind one ReLU.  Every stage is held to float64 from the fp32 values it read (its own bound); the end of the
    chain to float64 autograd of relu(sum batch_norm(x_i)) with bounds composed from the stages': the statistics' e(mean), e(invstd), e(a)
    carried through the backward (bn_ref.bn_backward's e_state).  The ReLU mask of the autograd graph is the kernel's own Y > 0; it has
    to agree with the float64 pre-activation wherever that lies further from 0 than MARGIN times its bound."""
    Xs = [R.columns(rows, C, 61 + i, first=i)[0] for i in range(n)]
    ps = [R.bn_params(C, 61 + i)[:4] + ((0.1, 1e-5), (0.3, 1e-3))[i] for i in range(n)]
    dY = torch.randn(rows, C, generator=R.gen_for(rows, C, 63))
    own = [run_stats(dev, X, p) for X, p in zip(Xs, ps)]
    refs = [R.train_stats(X, *p) for X, p in zip(Xs, ps)]
    for o, r, p in zip(own, refs, ps):
        check_state("chain stats", o, r, p, (rows, C))
    fwd = [(o["mean"], o["a"], o["b"]) for o in own]
    Y = run_affine(dev, 1, Xs[0], fwd[0], *((Xs[1], fwd[1]) if n == 2 else ()))
    flat = [t for X, s in zip(Xs, fwd) for t in (X,) + s]
    check("chain affine_act", "Y", Y, *R.affine_act(1, *flat), (rows, C))
    back = run_backward(dev, dY, Y, Xs, [(o["mean"], o["invstd"], o["a"]) for o in own])
    for i, (X, o) in enumerate(zip(Xs, own)):
        stage = R.bn_backward(dY, Y, X, o["mean"], o["invstd"], o["a"])
        for k in ("dgamma", "dbeta", "dX"):
            check("chain bn_backward", k, back["%s%d" % (k, i + 1)], *stage[k], (rows, C, i))
    # float64 autograd
    xs = [D(X).clone().requires_grad_(True) for X in Xs]
    gs = [D(p[0]).clone().requires_grad_(True) for p in ps]
    bs = [D(p[1]).clone().requires_grad_(True) for p in ps]
    pre = sum(F.batch_norm(x, None, None, g, b, True, 0.0, float(R.f32(p[5]))) for x, g, b, p in zip(xs, gs, bs, ps))
    e_pre = sum(R.affine_pre(X, r["mean"][0], r["a"][0], r["b"][0])[1] + r["a"][0].abs() * r["mean"][1] + (D(X) - r["mean"][0]).abs() * r["a"][1]
                for X, r in zip(Xs, refs))
    decided = pre.detach().abs() > MARGIN * e_pre
    assert bool(((Y > 0) == (pre.detach() > 0))[decided].all()), ("the kernel's mask is the float64 one wherever that is decided", rows, C)
    assert float(decided.double().mean()) > 0.6
    (pre * (Y > 0) * D(dY)).sum().backward()
    for i, (X, r, x, g, b) in enumerate(zip(Xs, refs, xs, gs, bs)):
        comp = R.bn_backward(dY, Y, X, r["mean"][0], r["invstd"][0], r["a"][0], e_state=(r["mean"][1], r["invstd"][1], r["a"][1]))
        for k, grad in (("dgamma", g.grad), ("dbeta", b.grad), ("dX", x.grad)):
            assert float((comp[k][0] - grad).abs().max()) <= 1e-9 * max(1.0, float(grad.abs().max())), ("the reference is autograd's", k)
            check("chain%d vs autograd" % n, k, back["%s%d" % (k, i + 1)], grad, comp[k][1], (rows, C, i))


@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=lambda c: "%d-%d" % c)
def test_chain_against_autograd(dev, case):
    check_chain(dev, *case, 1)


def test_chain_of_two_batchnorms_against_autograd(dev):
    check_chain(dev, *R.CHAIN_PAIR, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_colsum, _pair, mmego_colsum2
# ---------------------------------------------------------------------------------------------------------------------------------
def run_colsum(dev, Xw, rows, C, old=None, out2=False, scale=None):
    """-> {"out", "out2"}; Xw: a Wide holding X, or a (view, ld) pair."""
    view, ld = (Xw.view, Xw.ld) if isinstance(Xw, Wide) else Xw
    ws = vec_out(dev, C * R.nblk(rows))
    out, o2 = vec_out(dev, C, old), vec_out(dev, C) if out2 else None
    call("colsum", view, ld, rows, C, ws.view, out.view, o2.view if out2 else None, int(old is not None), None if scale is None else d_vec(dev, scale))
    assert intact(ws, out, o2) and (not isinstance(Xw, Wide) or Xw.guards_intact()), ("guards", rows, C)
    got = {"out": result(out)}
    if out2:
        got["out2"] = result(o2)
    return got


def check_colsum(dev, Xw, X, path, old, scale, note, long_path=False):
    """The four forms of one tensor: plain; out2; accumulate (the bits of old + plain, out2 receives the NEW value); and, on the short
    path, scale (the bits of plain * scale) and scale with accumulate (one of the two roundings may fuse: a bound)."""
    rows, C = X.shape
    k = path[0].replace("_kernel", "")
    base = twice(lambda: run_colsum(dev, Xw, rows, C))["out"]
    check(k, "out", base, *R.colsum(X, path), note)
    acc = twice(lambda: run_colsum(dev, Xw, rows, C, old, True))
    check(k, "out acc", acc["out"], *R.colsum(X, path, old), note)
    assert same_bits(acc["out"], old + base) and same_bits(acc["out2"], acc["out"]), ("accumulate: old + sum, and out2 receives it", note)
    two = run_colsum(dev, Xw, rows, C, None, True)
    assert same_bits(two["out"], base) and same_bits(two["out2"], base), ("out2 is out", note)
    if not long_path:
        sc = twice(lambda: run_colsum(dev, Xw, rows, C, None, True, scale))
        check(k, "out scale", sc["out"], *R.colsum(X, path, None, scale), note)
        assert same_bits(sc["out"], base * scale) and same_bits(sc["out2"], sc["out"]), ("scale: one product of the unscaled result", note)
        both = run_colsum(dev, Xw, rows, C, old, False, scale)
        check(k, "out acc scale", both["out"], *R.colsum(X, path, old, scale), note)
    return base


@pytest.mark.parametrize("rows", R.SHORT_ROWS)
def test_colsum_short(dev, rows):
    for C in R.SHORT_CS:
        X, old, scale = R.colsum_inputs(rows, C)
        path = R.colsum_path(rows, C, C + 3)
        assert path[0] == "colsum_small_kernel"
        check_colsum(dev, operand(dev, X, 3), X, path, old, scale, (rows, C))


@pytest.mark.parametrize("case", R.LONG_CASES, ids=lambda c: "-".join(str(v) for v in c[:4]))
def test_colsum_long(dev, case):
    rows, C, ld, lead, kernel = case
    X, old, scale = R.colsum_inputs(rows, C)
    Xw = Wide(dev, rows, C, ld, fill=NAN, src=X, lead=lead)
    path = R.colsum_path(rows, C, ld, Xw.view.data_ptr() % 16 == 0)
    assert path[0] == kernel and (Xw.view.data_ptr() % 16 == 0) == (lead == 0), case
    check_colsum(dev, Xw, X, path, old, scale, case, long_path=True)
    refused("colsum", Xw.view, ld, rows, C, torch.zeros(C * R.nblk(rows), device=dev), torch.zeros(C, device=dev), None, 0, d_vec(dev, scale))


def test_colsum_forms_agree(dev):
    """(4096, 256): the same values through colsum_partial4_kernel (aligned) and colsum_partial_kernel (one float past alignment; row
    stride 257), each within its bound of float64 and so within the sum of the bounds of each other."""
    rows, C = 4096, 256
    X, _, _ = R.colsum_inputs(rows, C)
    outs, bounds = [], []
    for ld, lead in ((260, 0), (260, 1), (257, 0)):
        Xw = Wide(dev, rows, C, ld, fill=NAN, src=X, lead=lead)
        path = R.colsum_path(rows, C, ld, lead == 0)
        outs.append(run_colsum(dev, Xw, rows, C)["out"])
        bounds.append(R.colsum(X, path)[1])
    assert same_bits(outs[1], outs[2])          # the same kernel, tile and order
    check("colsum forms", "out", outs[0], D(outs[1]), bounds[0] + bounds[1], (rows, C))


@pytest.mark.parametrize("rows", R.PAIR_SUM_ROWS)
def test_colsum_pair(dev, rows):
    """The two halves of X [rows][2 C] have the bits of two mmego_colsum calls (the same kernel, tile and order)."""
    for C in R.PAIR_SUM_CS:
        X, old, _ = R.colsum_inputs(rows, 2 * C)
        Xw = operand(dev, X, 3)
        for acc in (0, 1):
            for second in (False, True):
                def run():
                    o = {k: vec_out(dev, C, old[:C] if k == "A" else old[C:]) for k in ("A", "B")}
                    if second:
                        o.update({"A2": vec_out(dev, C), "B2": vec_out(dev, C)})
                    call("colsum_pair", Xw.view, Xw.ld, rows, C, o["A"].view, o["A2"].view if second else None, o["B"].view,
                         o["B2"].view if second else None, acc)
                    assert intact(Xw, *o.values()), ("guards", rows, C)
                    return {k: result(v) for k, v in o.items()}
                got = twice(run)
                for k, half in (("A", slice(0, C)), ("B", slice(C, 2 * C))):
                    one = run_colsum(dev, (Xw.view[:, half], Xw.ld), rows, C, old[half] if acc else None, True)
                    assert same_bits(got[k], one["out"]), ("colsum_pair is two colsums", rows, C, acc, k)
                    check("colsum_pair", "out" + k + (" acc" if acc else ""), got[k], *R.colsum(X[:, half], R.colsum_path(rows, C, Xw.ld), old[half] if acc else None),
                          (rows, C))
                    if second:
                        assert same_bits(got[k + "2"], got[k])


@pytest.mark.parametrize("case", R.COLSUM2_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_colsum2(dev, case):
    """Two short sums of different shapes in one launch; a one-column tensor has ld = 1 (a vector read as a column)."""
    rows1, C1, rows2, C2 = case
    X1, X2 = R.colsum_inputs(rows1, C1)[0], R.colsum_inputs(rows2, C2, 1)[0]
    w1 = operand(dev, X1, 3)
    w2 = Wide(dev, rows2, 1, 1, fill=NAN, src=X2) if C2 == 1 else operand(dev, X2, 5, col=2)

    def run():
        o1, o2 = vec_out(dev, C1), vec_out(dev, C2)
        call("colsum2", w1.view, w1.ld, rows1, C1, o1.view, w2.view, w2.ld, rows2, C2, o2.view)
        assert intact(w1, w2, o1, o2), ("guards", case)
        return {"out1": result(o1), "out2": result(o2)}
    got = twice(run)
    for k, X, w, rows, C in (("out1", X1, w1, rows1, C1), ("out2", X2, w2, rows2, C2)):
        check("colsum2", k, got[k], *R.colsum(X, R.colsum_path(rows, C, w.ld)), case)
        if C >= 16:          # mmego_colsum runs the 16-wide tile there too: the same order
            assert same_bits(got[k], run_colsum(dev, w, rows, C)["out"]), ("colsum2 is colsum where the tiles agree", case, k)


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_copy2d, _pair, mmego_relu_mask, mmego_fill: bits
# ---------------------------------------------------------------------------------------------------------------------------------
def payload(n):
    """n floats of many bit patterns: randn, +-0, denormals, NaN."""
    t = torch.randn(n, generator=R.gen_for(n, 71))
    for i, v in enumerate((0.0, -0.0, 1e-40, -1e-40, float("nan"), float("inf"))):
        t[i + 1::13] = v
    return t


@pytest.mark.parametrize("case", R.COPY_CASES, ids=lambda c: "%d-%d" % c)
def test_copy2d(dev, case):
    rows, C = case
    X = payload(rows * C).view(rows, C)
    Y0 = torch.randn(rows, C, generator=R.gen_for(rows, C, 72))
    Xw = operand(dev, X, 3)
    for acc in (0, 1):
        def run():
            Y = Wide(dev, rows, C, C + 5, col=2, src=Y0)
            call("copy2d", Xw.view, Xw.ld, Y.view, Y.ld, rows, C, acc)
            assert intact(Xw, Y)
            return {"Y": Y.cpu()}
        got = twice(run)["Y"]
        assert same_bits(got, X + Y0 if acc else X), ("copy2d", case, acc)


def test_copy2d_concatenates_128_and_45_columns(dev):
    """The 128 + 45 -> 173-column concatenation of nets.py: two copies into the column ranges of one buffer."""
    rows = 37
    A, B = payload(rows * 128).view(rows, 128), payload(rows * 45).view(rows, 45)
    Aw, Bw = operand(dev, A, 4, col=0), operand(dev, B, 3)
    Y = Wide(dev, rows, 173, 176, col=2)
    call("copy2d", Aw.view, Aw.ld, Y.view[:, :128], Y.ld, rows, 128, 0)
    call("copy2d", Bw.view, Bw.ld, Y.view[:, 128:], Y.ld, rows, 45, 0)
    assert same_bits(Y.cpu(), torch.cat((A, B), 1)) and intact(Y, Aw, Bw)


def test_copy2d_pair(dev):
    """A problem of 3 elements beside one above the 2048-block cap (the second problem's blocks walk their loop twice), and swapped."""
    big, small = R.COPY_CASES[-1], (1, 3)
    for (r1, c1), (r2, c2) in ((small, big), (big, small)):
        X1, X2 = payload(r1 * c1).view(r1, c1), payload(r2 * c2 + 1)[1:].view(r2, c2)
        w1, w2 = operand(dev, X1, 3), operand(dev, X2, 5, col=2)

        def run():
            Y1, Y2 = Wide(dev, r1, c1, c1 + 2, col=1), Wide(dev, r2, c2, c2 + 7, col=3)
            call("copy2d_pair", w1.view, w1.ld, Y1.view, Y1.ld, r1, c1, w2.view, w2.ld, Y2.view, Y2.ld, r2, c2)
            assert intact(w1, w2, Y1, Y2)
            return {"Y1": Y1.cpu(), "Y2": Y2.cpu()}
        got = twice(run)
        assert same_bits(got["Y1"], X1) and same_bits(got["Y2"], X2), ((r1, c1), (r2, c2))


@pytest.mark.parametrize("case", R.COPY_CASES, ids=lambda c: "%d-%d" % c)
def test_relu_mask(dev, case):
    """G becomes +0 where H fails `> 0` (H: +-0, negatives, NaN, denormals; G holds NaN exactly there) and keeps its bits elsewhere."""
    rows, C = case
    H = R.mask_values(rows, C, 73)
    keep = H > 0
    G0 = torch.where(keep, payload(rows * C).view(rows, C), torch.tensor(NAN))
    Hw = operand(dev, H, 3)

    def run():
        G = Wide(dev, rows, C, C + 5, col=2, src=G0)
        call("relu_mask", G.view, G.ld, Hw.view, Hw.ld, rows, C)
        assert intact(G, Hw)
        return {"G": G.cpu()}
    got = twice(run)["G"]
    assert same_bits(got, torch.where(keep, G0, torch.zeros(()))), ("relu_mask", case)
    if rows * C > 100:
        assert bool(keep.any()) and bool((~keep).any()) and bool((H[keep] < 1e-38).any())


@pytest.mark.parametrize("n", R.FILL_N)
def test_fill(dev, n):
    nan_payload = struct.unpack("f", struct.pack("I", 0x7FC12345))[0]
    for v in (1.5, -0.0, nan_payload):
        want = struct.unpack("i", struct.pack("f", ctypes.c_float(v).value))[0]
        X = vec_out(dev, n)
        call("fill", X.view, n, v)
        got = X.cpu().reshape(-1).view(torch.int32)
        assert bool((got == want).all()) and X.guards_intact(), (n, v)
    assert struct.unpack("I", struct.pack("f", ctypes.c_float(nan_payload).value))[0] == 0x7FC12345


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: the MMEGO_REQUIREs that stand before every launch of their entry point
# ---------------------------------------------------------------------------------------------------------------------------------
def each_refused(name, good, nulls, bad):
    """good: an argument list the entry point accepts (never launched here); each of `nulls` set to NULL and each (index, value) of
    `bad` must be refused."""
    for i in nulls:
        refused(name, *[None if j == i else a for j, a in enumerate(good)])
    for i, v in bad:
        refused(name, *[v if j == i else a for j, a in enumerate(good)])


def test_refusals(dev):
    t = torch.zeros(64 * 1024, device=dev)
    each_refused("bn_train_stats", [t, 8, 4, 8, t, t, t, t, 0.1, 1e-5, t, t, t, t, t], (0, 4, 5, 10, 11, 12, 13, 14),
                 ((2, 0), (2, -1), (3, 0), (6, None), (7, None)))
    each_refused("bn_finalize", [t, 4, 8, t, t, t, t, 0.1, 1e-5, t, t, t, t], (0, 3, 4, 9, 10, 11, 12),
                 ((1, 0), (1, 1025), (2, 0), (5, None), (6, None)))
    one = [t, 8, t, t, t, t, 0.1, 1e-5, t, t, t, t]
    each_refused("bn_train_stats_pair", [4, 8, t] + one + one, (2, 3, 5, 6, 11, 12, 13, 14, 15, 17, 18, 23, 24, 25, 26),
                 ((0, 0), (1, 0), (1, 24), (1, 65), (7, None), (8, None), (19, None), (20, None)))
    each_refused("bn_eval_affine", [8, t, t, t, t, 1e-5, t, t, t, t], (1, 2, 3, 4, 6, 7, 8, 9), ((0, 0),))
    each_refused("bn_fold_linear", [t, t, 4, 8, t, t, t, t, 1e-5, t, t], (0, 4, 5, 6, 7, 9, 10), ((2, 0), (3, 0)))
    each_refused("affine_act", [t, 8, t, t, t, t, 8, t, t, t, t, 8, 4, 8, 1], (0, 2, 3, 4, 7, 8, 9, 10), ((12, 0), (13, 0)))
    each_refused("affine_act", [t, 8, t, t, t, None, 0, None, None, None, t, 8, 4, 8, 1], (0, 2, 3, 4, 10), ((12, 0), (13, 0)))
    each_refused("copy2d", [t, 8, t, 8, 4, 8, 0], (0, 2), ((4, 0), (5, 0)))
    each_refused("copy2d_pair", [t, 8, t, 8, 4, 8, t, 8, t, 8, 4, 8], (0, 2, 6, 8), ((4, 0), (5, 0), (10, 0), (11, 0)))
    each_refused("bn_backward", [t, 8, t, 8, t, 8, t, t, t, 4, 8, t, t, t, t, t, 8], (0, 4, 6, 7, 8, 11, 12, 13, 14, 15), ((9, 0), (10, 0)))
    half = [t, 8, t, t, t, t, t, t, 8]
    each_refused("bn_backward_pair", [t, 8, t, 8, 4, 8, t, t] + half + half, (0, 6, 7, 8, 10, 11, 12, 13, 14, 15, 17, 19, 20, 21, 22, 23, 24),
                 ((4, 0), (5, 0), (5, 24), (5, 65)))
    each_refused("colsum", [t, 8, 4, 8, t, t, t, 0, None], (0, 4, 5), ((2, 0), (3, 0)))
    refused("colsum", t, 8, 1025, 8, t, t, None, 0, t)          # scale on the long path
    each_refused("colsum_pair", [t, 32, 4, 16, t, t, t, t, 0], (0, 4, 6), ((2, 0), (3, 0), (3, 8), (3, 24), (2, 1025)))
    each_refused("colsum2", [t, 8, 4, 8, t, t, 8, 4, 8, t], (0, 4, 5, 9), ((2, 0), (2, 1025), (3, 0), (7, 0), (7, 1025), (8, 0)))
    each_refused("relu_mask", [t, 8, t, 8, 4, 8], (0, 2), ((4, 0), (5, 0)))
    each_refused("fill", [t, 4, 1.0], (0,), ((1, 0),))
    assert bool((t == 0).all())
