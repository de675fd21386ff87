"""CPU: the float64 references, host rules, emulation and bounds of tests/bn_ref.py (what tests/test_bn_kernels_gpu.py holds csrc/bn.hip to).
  * the references are torch.nn.functional.batch_norm and its autograd in float64 (a condition on the reference, no measurement);
  * the restated host rules are the library's (mmego_colstats_nblk runs without a GPU) and every GPU case reaches the kernel it names;
  * the fp32 emulation, in the order the source fixes, stays inside MARGIN * bound on every case list of the GPU file, no element left out;
  * mutants of the EMULATION (no kernel is made wrong on a GPU) are held to the same references and bounds, and each one fails."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import bn_ref as R
from bn_ref import MARGIN, D

RATIOS = {}


def ratio(what, out, ref, bound):
    w = R.worst_ratio(out, ref, bound)[0]
    RATIOS[what] = max(RATIOS.get(what, 0.0), w)
    return w


def inside(what, out, ref, bound, note=""):
    w = ratio(what, out, ref, bound)
    assert w <= MARGIN, (what, note, w)


def close(a, b, tol=1e-12):
    a, b = D(a), D(b)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


@pytest.fixture(scope="module", autouse=True)
def table():
    yield
    print("\nlargest |emulation - ref| / bound per kernel and output (bound without MARGIN):")
    for k, v in sorted(RATIOS.items()):
        print("EMU %-34s %.4g" % (k, v))


# ---------------------------------------------------------------------------------------------------------------------------------
# the references are torch's
# ---------------------------------------------------------------------------------------------------------------------------------
def torch_bn(x, p, mom, eps, training=True):
    gamma, beta, rm, rv = (D(t).clone() for t in p)
    x = D(x).clone().requires_grad_(True)
    gamma.requires_grad_(True)
    beta.requires_grad_(True)
    y = F.batch_norm(x, rm, rv, gamma, beta, training, float(torch.tensor(mom, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32)))
    return x, gamma, beta, rm, rv, y


@pytest.mark.parametrize("relu", (0, 1))
def test_train_references_are_torch(relu):
    rows, C, mom, eps = 37, 13, 0.1, 1e-5
    X, _ = R.columns(rows, C, 1)
    X = X * 0.01 + torch.randn(rows, C, generator=R.gen_for(5)) if relu else X
    p = R.bn_params(C, 1)
    x, g, b, rm, rv, y = torch_bn(X, p, mom, eps)
    st = R.train_stats(X, *p, mom, eps)
    close(st["running_mean"][0], rm)
    close(st["running_var"][0], rv)
    ours = R.affine_act(relu, X, st["mean"][0], st["a"][0], st["b"][0])[0]
    out = torch.relu(y) if relu else y
    close(ours, out.detach(), 1e-11)
    dY = torch.randn(rows, C, generator=R.gen_for(6), dtype=torch.float64)
    (out * dY).sum().backward()
    back = R.bn_backward(dY, out.detach() if relu else None, X, st["mean"][0], st["invstd"][0], st["a"][0])
    close(back["dX"][0], x.grad, 1e-10)
    close(back["dgamma"][0], g.grad, 1e-10)
    close(back["dbeta"][0], b.grad, 1e-10)


def test_two_batchnorms_behind_one_relu_are_torch():
    rows, C = 37, 16
    X1, X2 = R.columns(rows, C, 2)[0] * 0.01, torch.randn(rows, C, generator=R.gen_for(7))
    p1, p2 = R.bn_params(C, 2), R.bn_params(C, 3)
    x1, g1, b1, _, _, y1 = torch_bn(X1, p1, 0.1, 1e-5)
    x2, g2, b2, _, _, y2 = torch_bn(X2, p2, 0.3, 1e-3)
    s1, s2 = R.train_stats(X1, *p1, 0.1, 1e-5), R.train_stats(X2, *p2, 0.3, 1e-3)
    out = torch.relu(y1 + y2)
    ours = R.affine_act(1, X1, s1["mean"][0], s1["a"][0], s1["b"][0], X2, s2["mean"][0], s2["a"][0], s2["b"][0])[0]
    close(ours, out.detach(), 1e-9)
    dY = torch.randn(rows, C, generator=R.gen_for(8), dtype=torch.float64)
    (out * dY).sum().backward()
    for X, s, x, g, b in ((X1, s1, x1, g1, b1), (X2, s2, x2, g2, b2)):
        back = R.bn_backward(dY, out.detach(), X, s["mean"][0], s["invstd"][0], s["a"][0])
        close(back["dX"][0], x.grad, 1e-9)
        close(back["dgamma"][0], g.grad, 1e-9)
        close(back["dbeta"][0], b.grad, 1e-9)


def test_eval_references_are_torch():
    C, K, eps = 13, 7, 1e-3
    p = R.bn_params(C, 4)
    X = torch.randn(9, C, generator=R.gen_for(9))
    _, _, _, _, _, y = torch_bn(X, p, 0.1, eps, training=False)
    st = R.eval_affine(*p, eps)
    close(R.affine_act(0, X, st["mean"][0], st["a"][0], st["b"][0])[0], y.detach())
    W, b, xin = (torch.randn(*s, generator=R.gen_for(10)) for s in ((C, K), (C,), (9, K)))
    for bias in (b, None):
        fold = R.fold_linear(W, bias, *p, eps)
        pre = D(xin) @ D(W).t() + (0.0 if bias is None else D(bias))
        want = F.batch_norm(pre, D(p[2]), D(p[3]), D(p[0]), D(p[1]), False, 0.1, float(torch.tensor(eps, dtype=torch.float32)))
        close(D(xin) @ fold["Wf"][0].t() + fold["bf"][0], want)


def test_single_row_takes_the_biased_variance():
    """N == 1: torch has NaN for the unbiased variance; the kernel's rule is the biased value, 0."""
    X, _ = R.columns(1, 6, 3)
    p = R.bn_params(6, 5)
    st = R.train_stats(X, *p, 0.1, 1e-5)
    close(st["running_var"][0], 0.9 * D(p[3]), 1e-7)
    assert bool((st["invstd"][0] == 1.0 / torch.sqrt(torch.tensor(float(torch.tensor(1e-5, dtype=torch.float32)), dtype=torch.float64))).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# host rules
# ---------------------------------------------------------------------------------------------------------------------------------
def test_host_rules_are_the_library_s():
    from mmego_amd import build
    lib = ctypes.CDLL(build.build_library())
    for rows in list(range(1, 5001)) + [16384, 16385, 1048576]:
        assert lib.mmego_colstats_nblk(ctypes.c_long(rows)) == R.nblk(rows), rows
        assert R.nblk(rows) <= 1024 and R.rows_per_block(rows) % 4 == 0
    assert (R.rows_per_block(16385), R.nblk(16385), 16385 - 819 * 20) == (20, 820, 5)
    assert [R.col_tile(c) for c in R.CS] == [8, 8, 8, 32, 64, 64, 64, 64] and R.col_tile(16) == 16 and R.col_tile(128) == 64
    assert [R.short_tile(c) for c in R.SHORT_CS] == [8, 8, 8, 16, 16, 16, 16, 16]
    assert R.ew_blocks(R.EW_CAP) == 2048 and R.ew_passes(R.EW_CAP) == 1 and R.ew_passes(R.EW_CAP + 1) == 2 and R.ew_blocks(1) == 1


def test_every_case_reaches_what_it_names():
    # statistics and backward: every column tile, one block and many, a last block shorter than TR, the 820-block case
    tiles = {R.col_tile(c[1]) for c in R.STATS_CASES}
    assert tiles == {8, 32, 64} and {R.col_tile(c) for _, c in R.PAIR_CASES} == {8, 16, 64}
    assert {R.col_tile(c[1]) for c in R.BWD_CASES} == {8, 32, 64}
    assert (37 % R.rows_per_block(37)) < 256 // R.col_tile(27) and R.nblk(37) == 3          # 5 rows in the last block, TR = 8
    assert R.nblk(1024) == 64 and R.nblk(1025) == 65 and R.nblk(16) == 1 and R.nblk(17) == 2
    assert all(c % R.col_tile(c) == 0 for _, c in R.PAIR_CASES + R.BWD_PAIR_CASES)
    # colsum
    for rows in R.SHORT_ROWS:
        for C in R.SHORT_CS:
            assert R.colsum_path(rows, C, C + 3)[0] == "colsum_small_kernel"
    for TR in (16, 32):      # the 4-deep unroll: lanes with 0, 1, 3, 4 and 5 rows
        assert {min(5, R.cdiv(max(r - ry, 0), TR)) for r in R.SHORT_ROWS for ry in range(TR)} >= {0, 1, 3, 4, 5}
    for rows, C, ld, lead, kernel in R.LONG_CASES:
        assert R.colsum_path(rows, C, ld, lead == 0)[0] == kernel, (rows, C, ld, lead)
    assert R.colsum_path(1024, 256, 256)[0] == "colsum_small_kernel" and R.colsum_path(1025, 256, 256)[0] == "colsum_partial_kernel"
    assert R.colsum_path(4100, 260, 264)[2:] == (128, 33) and 4100 % 128 == 4 and 260 % 64 == 4
    rows, C = R.LONG_BLOCKS_RULE
    assert R.cdiv(rows, 128) > R.nblk(rows) and R.colsum_path(rows, C, C)[0] == "colsum_partial_kernel"
    assert R.colsum_path(131072, C, C)[0] == "colsum_partial4_kernel"
    # the elementwise grid walks its loop a second time
    assert R.ew_passes(R.FOLD_CASES[-1][0] * R.FOLD_CASES[-1][1]) == 2 and R.ew_passes(R.AFFINE_CASES[-1][0] * R.AFFINE_CASES[-1][1]) == 2
    assert R.ew_passes(R.COPY_CASES[-1][0] * R.COPY_CASES[-1][1]) == 2 and R.ew_passes(R.FILL_N[-1]) == 2 and R.ew_passes(R.FILL_N[-2]) == 1
    assert R.ew_passes(16385 * 45) == 2          # bn_bwd_apply_kernel
    # every kind of column in every colsum case: the cancelling column is column 0
    assert int(R.columns(5, 1, 0, first=R.CANCEL)[1][0]) == R.CANCEL


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation stays inside the bounds on every case list of the GPU file
# ---------------------------------------------------------------------------------------------------------------------------------
stats_inputs, colsum_inputs = R.stats_inputs, R.colsum_inputs


@pytest.mark.parametrize("case", R.STATS_CASES, ids=lambda c: "%d-%d" % c[:2])
def test_emulated_train_stats_inside_bounds(case):
    X, kinds, p = stats_inputs(case)
    ref, emu = R.train_stats(X, *p), R.emu_train_stats(X, *p)
    assert set(ref) == set(emu) and len(ref) == (6 if case[2] else 4)
    for k in ref:
        assert emu[k].shape == ref[k][0].shape == (case[1],)
        inside("bn_train_stats " + k, emu[k], *ref[k], case)
    const = kinds == 2
    assert bool((emu["invstd"][const] == (1.0 / torch.sqrt(R.f32(case[4]).double())).float()).all())
    if case[2] and case[3] == 0.0:
        assert R.same_bits(emu["running_mean"], p[2]) and R.same_bits(emu["running_var"], p[3])
    if case[2] and case[3] == 1.0:
        assert torch.equal(emu["running_mean"], emu["mean"])


@pytest.mark.parametrize("nb", R.FINALIZE_NBLK)
def test_emulated_finalize_inside_bounds(nb):
    rec, p = R.hand_records(nb, 5, 1), R.bn_params(5, 12)
    ref, emu = R.finalize(*rec, *p, 0.1, 1e-5), R.emu_finalize(*rec, *p, 0.1, 1e-5)
    for k in ref:
        inside("bn_finalize " + k, emu[k], *ref[k], nb)


@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: "%d-%d" % c[:2])
def test_emulated_backward_inside_bounds(case):
    rows, C, masked = case
    X, _ = R.columns(rows, C, 13)
    dY, M = torch.randn(rows, C, generator=R.gen_for(rows, C, 14)), R.mask_values(rows, C, 13) if masked else None
    st = R.given_state(C, 13)
    ref, emu = R.bn_backward(dY, M, X, *st), R.emu_bn_backward(dY, M, X, *st)
    for k, o in zip(("dgamma", "dbeta", "dX"), emu):
        assert o.shape == ref[k][0].shape
        inside("bn_backward " + k, o, *ref[k], case)


def test_emulated_colsum_inside_bounds():
    shapes = [(r, c, c + 3, 0) for r in R.SHORT_ROWS for c in R.SHORT_CS] + [c[:4] for c in R.LONG_CASES]
    for rows, C, ld, lead in shapes:
        X, old, scale = colsum_inputs(rows, C)
        path = R.colsum_path(rows, C, ld, lead == 0)
        short = path[0] == "colsum_small_kernel"
        for o, s in ((None, None), (old, None)) + (((None, scale), (old, scale)) if short else ()):
            out, out2 = R.emu_colsum(X, path, o, s)
            assert R.same_bits(out, out2) and out.shape == (C,)
            inside(path[0].replace("_kernel", "") + (" acc" if o is not None else "") + (" scale" if s is not None else ""), out,
                   *R.colsum(X, path, o, s), (rows, C, ld, lead))


def test_emulated_seg_form_inside_bounds():
    """colsum_small_kernel with seg (mmego_colsum_pair) has the bits of two single calls; with seg AND scale (no entry point passes
    both: the kernel's own rule, out[c] = sum * scale[c]) it is held to float64."""
    for rows in R.PAIR_SUM_ROWS:
        for C in R.PAIR_SUM_CS:
            X, old, scale = colsum_inputs(rows, 2 * C)
            A, A2, B, B2 = R.emu_colsum_small(X, 16, (old[:C], old[C:]), None, C)
            for half, o, o2 in ((slice(0, C), A, A2), (slice(C, 2 * C), B, B2)):
                one = R.emu_colsum(X[:, half], R.colsum_path(rows, C, 2 * C), old[half])
                assert R.same_bits(o, one[0]) and R.same_bits(o2, one[1])
            A, _, B, _ = R.emu_colsum_small(X, 16, None, scale, C)
            inside("colsum_small seg scale", torch.cat((A, B)), *R.colsum(X, R.colsum_path(rows, 2 * C, 2 * C), None, scale), (rows, C))


def test_emulated_pair_and_colsum2_cases_inside_bounds():
    """The pair forms run the single forms' arithmetic on each half: their case lists through the same emulation."""
    for rows, C in R.PAIR_CASES:
        for key, mom, eps in ((21, 0.1, 1e-5), (22, 0.3, 1e-3)):
            X, p = R.columns(rows, C, key, first=3 * (key - 21))[0], R.bn_params(C, key) + (mom, eps)
            ref, emu = R.train_stats(X, *p), R.emu_train_stats(X, *p)
            for k in ref:
                inside("bn_train_stats_pair " + k, emu[k], *ref[k], (rows, C))
    for rows, C in R.BWD_PAIR_CASES:
        dY, M = torch.randn(rows, C, generator=R.gen_for(rows, C, 17)), R.mask_values(rows, C, 15)
        for key in (15, 16):
            X, st = R.columns(rows, C, key, first=2 * (key - 15))[0], R.given_state(C, key)
            ref = R.bn_backward(dY, M, X, *st)
            for k, o in zip(("dgamma", "dbeta", "dX"), R.emu_bn_backward(dY, M, X, *st)):
                inside("bn_backward_pair " + k, o, *ref[k], (rows, C))
    for rows1, C1, rows2, C2 in R.COLSUM2_CASES:
        for X in (colsum_inputs(rows1, C1)[0], colsum_inputs(rows2, C2, 1)[0]):
            inside("colsum2", R.emu_colsum_small(X, 16)[0], *R.colsum(X, R.colsum_path(*X.shape, X.shape[1])), X.shape)


def test_fp32_elementwise_forms_inside_bounds():
    """bn_eval_affine, bn_fold_linear and affine_act evaluated in unfused fp32 (the kernels may fuse one product and sum each)."""
    for C in R.EVAL_C:
        g, b, rm, rv = R.bn_params(C, 31)
        rv[C // 2] = 0.0
        inv = 1.0 / torch.sqrt(rv + R.f32(1e-5))
        ref = R.eval_affine(g, b, rm, rv, 1e-5)
        inside("bn_eval_affine invstd", inv, *ref["invstd"], C)
        inside("bn_eval_affine a", g * inv, *ref["a"], C)
    for N, K in R.FOLD_CASES:
        gen = R.gen_for(N, K, 33)
        W, b = torch.randn(N, K, generator=gen), torch.randn(N, generator=gen)
        g, be, rm, rv = R.bn_params(N, 33)
        s = g / torch.sqrt(rv + R.f32(1e-5))
        ref = R.fold_linear(W, b, g, be, rm, rv, 1e-5)
        inside("bn_fold_linear Wf", s[:, None] * W, *ref["Wf"], (N, K))
        inside("bn_fold_linear bf", (b - rm) * s + be, *ref["bf"], (N, K))
    for rows, C in R.AFFINE_CASES:
        X1, X2 = R.columns(rows, C, 35)[0], torch.randn(rows, C, generator=R.gen_for(rows, C, 36))
        (m1, _, a1), (m2, _, a2) = R.given_state(C, 35), R.given_state(C, 36)
        b1 = b2 = torch.randn(C, generator=R.gen_for(C, 3)) * 0.3
        v1 = (X1 - m1) * a1 + b1
        inside("affine_act Y", v1, *R.affine_act(0, X1, m1, a1, b1), (rows, C))
        inside("affine_act Y two relu", (v1 + ((X2 - m2) * a2 + b2)).clamp_min(0.0), *R.affine_act(1, X1, m1, a1, b1, X2, m2, a2, b2), (rows, C))


@pytest.mark.parametrize("case", R.CHAIN_CASES + (R.CHAIN_PAIR,), ids=lambda c: "%d-%d" % c)
def test_emulated_chain_inside_composed_bounds(case):
    """statistics -> affine + ReLU -> backward, every stage in fp32 from the stage before: the end of the chain against the float64
    backward of the float64 statistics, inside the bounds composed from e(mean), e(invstd), e(a) (bn_backward's e_state).  The mask is
    the fp32 chain's own Y > 0."""
    rows, C = case
    X, p = R.columns(rows, C, 61)[0], R.bn_params(C, 61) + (0.1, 1e-5)
    dY = torch.randn(rows, C, generator=R.gen_for(rows, C, 63))
    own, r = R.emu_train_stats(X, *p), R.train_stats(X, *p)
    Y = ((X - own["mean"]) * own["a"] + own["b"]).clamp_min(0.0)
    got = R.emu_bn_backward(dY, Y, X, own["mean"], own["invstd"], own["a"])
    comp = R.bn_backward(dY, Y, X, r["mean"][0], r["invstd"][0], r["a"][0], e_state=(r["mean"][1], r["invstd"][1], r["a"][1]))
    for k, o in zip(("dgamma", "dbeta", "dX"), got):
        inside("chain vs float64 " + k, o, *comp[k], case)


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants of the emulation: each is held to the references and bounds above, and fails
# ---------------------------------------------------------------------------------------------------------------------------------
def worst_stats(cases, mutant, keys):
    w = 0.0
    for case in cases:
        X, _, p = stats_inputs(case)
        ref, emu = R.train_stats(X, *p), R.emu_train_stats(X, *p, mutant=mutant)
        w = max([w] + [R.worst_ratio(emu[k], *ref[k])[0] for k in keys if k in ref])
    return w


def test_mutated_emulations_fail():
    far, stats = {}, [c for c in R.STATS_CASES if c[0] in (37, 1025) and c[1] in (27, 65)]
    # name: (ratio of the mutant, the comparison that catches it)
    far["no block shift"] = (worst_stats(stats, "no shift", ("invstd",)), "bn_train_stats invstd (large-mean column)")
    far["M2 / N for the running variance"] = (worst_stats(stats, "biased running var", ("running_var",)), "bn_train_stats running_var")
    far["momentum on the old value"] = (worst_stats(stats, "momentum on the old value", ("running_mean",)), "bn_train_stats running_mean")
    far["last partial block dropped"] = (worst_stats(stats, "drop last block", ("mean",)), "bn_train_stats mean")
    far["lanes k >= nblk not zeroed"] = (worst_stats(stats, "lanes not zeroed", ("mean",)), "bn_train_stats mean")
    rec, p = R.hand_records(65, 5, 1), R.bn_params(5, 12)
    ref = R.finalize(*rec, *p, 0.1, 1e-5)
    far["lanes k >= nblk not zeroed (finalize)"] = (R.worst_ratio(R.emu_finalize(*rec, *p, 0.1, 1e-5, "lanes not zeroed")["invstd"], *ref["invstd"])[0],
                                                    "bn_finalize invstd")
    # the second BatchNorm of a pair reads the first one's X
    X1, X2 = R.columns(37, 16, 21)[0], R.columns(37, 16, 22, first=1)[0]
    p2 = R.bn_params(16, 22)
    far["second of a pair reads the first X"] = (R.worst_ratio(R.emu_train_stats(X1, *p2, 0.1, 1e-5)["mean"], *R.train_stats(X2, *p2, 0.1, 1e-5)["mean"])[0],
                                                 "bn_train_stats_pair mean2")
    rows, C = 37, 27
    X, _ = R.columns(rows, C, 13)
    dY, M, st = torch.randn(rows, C, generator=R.gen_for(rows, C, 14)), R.mask_values(rows, C, 13), R.given_state(C, 13)
    ref = R.bn_backward(dY, M, X, *st)
    assert bool((M == 0).any())
    for name, mutant, k, i in (("mask >= 0", "mask >= 0", "dbeta", 1), ("c1, c2 over rows - 1", "rows - 1", "dX", 2), ("dX without xhat c2", "no xhat c2", "dX", 2)):
        far[name] = (R.worst_ratio(R.emu_bn_backward(dY, M, X, *st, mutant=mutant)[i], *ref[k])[0], "bn_backward " + k)
    rows, C = 65, 32
    X, old, scale = colsum_inputs(rows, 2 * C)
    path = R.colsum_path(rows, 2 * C, 2 * C)
    far["out2 before accumulation"] = (R.worst_ratio(R.emu_colsum(X, path, old, None, "out2 before accumulation")[1], *R.colsum(X, path, old))[0], "colsum out2 acc")
    A, _, B, _ = R.emu_colsum_small(X, 16, None, scale, C, "scale[cc]")
    far["scale[cc] for scale[c]"] = (R.worst_ratio(torch.cat((A, B)), *R.colsum(X, path, None, scale))[0], "colsum_small seg scale (emulation only)")
    A, _, B, _ = R.emu_colsum_small(X, 16, None, None, C, "seg off by one tile")
    far["seg boundary off by one tile"] = (R.worst_ratio(torch.cat((A, B)), *R.colsum(X, path))[0], "colsum_pair outB")
    Xl = colsum_inputs(4100, 260)[0]
    pl = R.colsum_path(4100, 260, 264)
    far["last partial block dropped (colsum)"] = (R.worst_ratio(R.emu_colsum(Xl, pl, mutant="drop last block")[0], *R.colsum(Xl, pl))[0], "colsum_partial4 out")
    print("\n" + "\n".join("MUTANT %-40s ratio %-10.3g caught by %s" % (k, v[0], v[1]) for k, v in far.items()))
    for k, (v, _) in far.items():
        assert v > 8 * MARGIN, (k, v)
