"""CPU: the float64 references and bounds of tests/pool_ref.py, before any GPU sees them.

  * the references ARE float64 torch.softmax / matmul and their float64 autograd (1e-12);
  * an fp32 emulation of every kernel form stays inside every bound WITHOUT the margin (ratio <= 1) at every shape and row kind of
    tests/test_pool_kernels_gpu.py;
  * host-side mirrors of mmego_attn_pool_forward's and _backward's kernel choice and of the LDS kernels' work split, held to the text of
    csrc/pool.hip, pin that the GPU file's cases reach every kernel and inner branch they claim to;
  * mutants of the emulation land far outside the bounds."""
import os

import pytest
import torch

import pool_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmego_amd", "csrc")


def inside(what, out, ref, bound):
    r, idx = R.worst_ratio(out, ref, bound)
    assert r <= 1.0, "%s: emulation / bound ratio %.3g at %s" % (what, r, idx)
    return r


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# agreement with torch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_b", (True, False))
def test_attention_pooling_reference_is_torch(with_b):
    G, P, C = 3, 11, 20
    I = R.pool_inputs(G, P, C, 0 if with_b else 1)
    X, w = I["X"].double().requires_grad_(True), I["w"].double().requires_grad_(True)
    b = torch.tensor(0.0 if I["b"] is None else I["b"], dtype=torch.float64, requires_grad=True)
    a = torch.softmax(X @ w + b, -1)
    vec = torch.einsum("gp,gpc->gc", a, X)
    ref = R.attn_pool_fwd(I["X"], I["w"], I["b"])
    assert close(ref["attn"][0], a.detach()) and close(ref["vec"][0], vec.detach())
    # dX is the whole gradient: a_p dvec through the weighted sum, ds_p w through the scores
    vec.backward(I["dvec"].double())
    back = R.attn_pool_bwd(I["X"], I["w"], a.detach(), I["dvec"])
    assert close(back["dX"][0], X.grad) and close(back["pdw"][0].sum(0), w.grad) and close(back["pdb"][0].sum(), b.grad)


def test_cross_attention_reference_is_torch():
    I = R.cross_inputs(3)
    Q, K, V = (I[k].double().requires_grad_(True) for k in ("Q", "K", "V"))
    Pm = torch.softmax(Q @ K.transpose(1, 2) * I["scale"], -1)
    O = Pm @ V
    ref = R.cross_fwd(I["Q"], I["K"], I["V"], I["scale"])
    assert close(ref["P"][0], Pm.detach()) and close(ref["O"][0], O.detach()) and close(ref["osum"][0], O.detach().sum(1))
    O.backward(I["dO"].double())
    back = R.cross_bwd(I["Q"], I["K"], I["V"], Pm.detach(), I["dO"], I["scale"])
    assert close(back["dQ"][0], Q.grad) and close(back["dK"][0], K.grad) and close(back["dV"][0], V.grad)
    J = R.cross_inputs(2, proj=True)
    q, _ = R.query_proj(J["X"], J["Wq"], J["bq"])
    assert close(q, torch.nn.functional.linear(J["X"].double(), J["Wq"].double(), J["bq"].double())) and bool((q[..., 0] == 4.0).all())


def test_group_references_are_torch():
    X, dY = R.sum_inputs(3, 9, 5)
    assert close(R.group_sum(X, 0.25)[0], X.double().sum(1) * 0.25)
    assert close(R.group_bcast(dY, 9, 0.5, X)[0], X.double() + 0.5 * dY.double()[:, None, :])


def test_row_kinds_are_what_they_claim():
    """Saturated groups have weights exactly 0 and 1 in fp32, tied groups exactly 1 / P, the near -100 groups scores below -90."""
    I = R.pool_inputs(5, 33, 64)
    ref = R.attn_pool_fwd(I["X"], I["w"], I["b"])
    s, a = ref["s"][0], ref["attn"][0].float()
    top = s.sort(-1).values
    assert 25 < float(top[1, -1] - top[1, -2]) < 35 and 190 < float(top[2, -1] - top[2, -2]) < 210
    assert sorted(a[2].tolist())[-2:] == [0.0, 1.0] and float(a[1].max()) == 1.0 and float(a[1].min()) > 0.0
    assert bool((s[3] == s[3, 0]).all()) and bool((a[3] == torch.tensor(1.0 / 33).float()).all()) and float(s[4].max()) < -90
    J = R.cross_inputs(8)
    Pm = R.cross_fwd(J["Q"], J["K"], J["V"], J["scale"])["P"][0]
    assert bool((Pm[1].argmax(-1) == 14).all()) and bool((Pm[2].argmax(-1) == 0).all()) and bool((Pm[7].float()[:, 14] == 1.0).all())
    assert bool((Pm[7].float()[:, :14] == 0.0).all()) and float((Pm[4] - 1.0 / 15).abs().max()) < 1e-15 and float(Pm[1][:, 14].min()) > 0.999


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation stays inside the bounds (no MARGIN)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: "-".join(str(v) for v in c[:4]))
def test_emulated_attn_pool_forward_inside_bounds(case):
    P, C, G, off, kernel = case
    for shift in R.shifts(G):
        I = R.pool_inputs(G, P, C, shift)
        ref = R.attn_pool_fwd(I["X"], I["w"], I["b"])
        a, vec = R.emu_attn_pool_fwd(I["X"], I["w"], I["b"], kernel)
        inside("attn", a, *ref["attn"])
        inside("vec", vec, *ref["vec"])
        tied = I["kinds"] == 3
        assert bool((a[tied] == torch.tensor(1.0 / P).float()).all())


@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: "-".join(str(v) for v in c[:4]))
def test_emulated_attn_pool_backward_inside_bounds(case):
    P, C, G, off, kernel = case
    for shift in R.shifts(G):
        I = R.pool_inputs(G, P, C, shift)
        attn = R.attn_pool_fwd(I["X"], I["w"], I["b"])["attn"][0].float()
        ref = R.attn_pool_bwd(I["X"], I["w"], attn, I["dvec"])
        dX, pdw, pdb = R.emu_attn_pool_bwd(I["X"], I["w"], attn, I["dvec"], kernel)
        inside("dX", dX, *ref["dX"])
        inside("pdw", pdw, *ref["pdw"])
        inside("pdb", pdb, *ref["pdb"])


@pytest.mark.parametrize("F", R.CROSS_F)
def test_emulated_cross_attention_inside_bounds(F):
    for shift in R.shifts(F, 8):
        I = R.cross_inputs(F, shift)
        ref = R.cross_fwd(I["Q"], I["K"], I["V"], I["scale"])
        for form in ("scalar", "mfma"):
            Pm, O = R.emu_cross_fwd(I["Q"], I["K"], I["V"], I["scale"], form)
            inside("P " + form, Pm, *ref["P"])
            inside("O " + form, O, *ref["O"])
            inside("osum " + form, R.emu_rows_sum(O, 1.0), *ref["osum"])
        Pg = ref["P"][0].float()
        for scale in (0.125, 1.0):
            back = R.cross_bwd(I["Q"], I["K"], I["V"], Pg, I["dO"], scale)
            for k, v in zip(("dQ", "dK", "dV"), R.emu_cross_bwd(I["Q"], I["K"], I["V"], Pg, I["dO"], scale)):
                inside(k, v, *back[k])


def test_emulated_pooled_q_inside_bounds():
    I = R.cross_inputs(R.POOLED_Q_F, proj=True)
    q, e_q = R.query_proj(I["X"], I["Wq"], I["bq"])
    ref = R.cross_fwd(q, I["K"], I["V"], I["scale"], e_q)
    q32 = I["X"] @ I["Wq"].t() + I["bq"]
    inside("Q", q32, q, e_q)
    _, O = R.emu_cross_fwd(q32, I["K"], I["V"], I["scale"], "mfma")
    inside("osum", R.emu_rows_sum(O, 1.0), *ref["osum"])


def test_emulated_group_sums_inside_bounds():
    for P in R.SUM_P:
        for G, C in R.SUM_GC:
            X, dY = R.sum_inputs(G, P, C)
            inside("group_sum", R.emu_rows_sum(X, 1.0 / P), *R.group_sum(X, 1.0 / P))
            inside("group_bcast", R.emu_group_bcast(dY, P, 0.75), *R.group_bcast(dY, P, 0.75))
            inside("group_bcast +", R.emu_group_bcast(dY, P, 0.75, X), *R.group_bcast(dY, P, 0.75, X))


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch mirrors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_dispatch_tables_reach_every_kernel_and_branch():
    fwd = {(P, C, off): k for P, C, G, off, k in R.FWD_CASES}
    for (P, C, off), want in fwd.items():
        assert R.fwd_kernel(P, C, not off) == want, (P, C, off)
    reg20 = {pc[:2] for pc, k in fwd.items() if k == "attn_pool_fwd_reg_kernel<20>"}
    reg32 = {pc[:2] for pc, k in fwd.items() if k == "attn_pool_fwd_reg_kernel<32>"}
    assert reg20 == {(1, 4), (7, 36), (20, 1020), (20, 1024)} and reg32 == {(21, 64), (32, 1024)}
    inner = {pc[:2]: R.fwd_lds_inner(*pc[:2]) for pc, k in fwd.items() if k == "attn_pool_fwd_lds_kernel"}
    pick = lambda pc, *keys: tuple(inner[pc][k] for k in keys)
    assert pick((33, 64), "TPP", "len", "wide", "PG", "wl", "NQ") == (4, 16, True, 4, True, 4)
    assert pick((128, 64), "TPP", "wide", "PG", "NQ") == (2, True, 4, 8)
    assert pick((100, 128), "TPP", "wide", "PG", "NQ") == (2, True, 2, 16)
    assert pick((300, 12), "TPP", "wide", "PG", "NQ") == (1, True, 1, 4)                     # 256 % 12 != 0
    assert pick((5, 1028), "TPP", "len", "wide", "PG", "wl", "NQ") == (4, 257, True, 1, False, 8)
    assert pick((1100, 8), "TPP", "wide", "PG", "NQ") == (1, False, 32, 16)
    assert pick((96, 252), "TPP", "wide", "PG", "NQ", "tile") == (2, True, 1, 24, 97152) and inner[(96, 252)]["tile"] <= 96 * 1024
    assert inner[(96, 252)]["lds"] == 105376 <= 160 * 1024                                   # with the static arrays: inside a CU's 160 KB
    plain = {pc for pc, k in fwd.items() if k == "attn_pool_fwd_kernel"}
    assert plain == {(50, 30, 0), (128, 256, 0), (20, 64, 1), (8192, 3, 0)}
    assert R.fwd_lds_inner(128, 256)["tile"] > 96 * 1024 and R.fwd_kernel(20, 64) == "attn_pool_fwd_reg_kernel<20>"
    assert {G for P, C, G, off, k in R.FWD_CASES if (P, C) == (7, 36)} == {1, 3, 257} == {G for P, C, G, off, k in R.FWD_CASES if (P, C) == (33, 64)}

    bwd = {(P, C, off): k for P, C, G, off, k in R.BWD_CASES}
    for (P, C, off), want in bwd.items():
        assert R.bwd_kernel(P, C, not off) == want, (P, C, off)
    binner = {pc[:2]: R.bwd_lds_inner(*pc[:2]) for pc, k in bwd.items() if k == "attn_pool_bwd_lds_kernel"}
    bpick = lambda pc, *keys: tuple(binner[pc][k] for k in keys)
    assert bpick((1, 4), "TPP", "len", "wide", "TCc", "PG", "NQ") == (4, 1, True, 4, 64, 2)
    assert bpick((33, 16), "TPP", "wide", "TCc", "PG", "NQ") == (4, True, 16, 16, 2)
    assert bpick((128, 64), "TPP", "wide", "TCc", "PG", "NQ") == (2, True, 64, 4, 8)
    assert bpick((20, 256), "TPP", "wide", "TCc", "PG", "NQ") == (8, True, 256, 1, 8)
    assert bpick((1100, 8), "TPP", "wide", "TCc", "PG", "NQ") == (1, False, 8, 32, 16)
    assert bpick((120, 128), "TPP", "wide", "PG", "NQ", "tile", "lds") == (2, True, 2, 16, 63424, 71648)
    assert binner[(120, 128)]["tile"] <= 64 * 1024 < binner[(120, 128)]["lds"]               # the launch that needs the raised limit
    assert {pc for pc, k in bwd.items() if k == "attn_pool_bwd_kernel"} == {(20, 1024, 0), (40, 12, 0), (50, 30, 0), (128, 64, 1)}
    assert R.bwd_tile(20, 1024) > 64 * 1024 and 256 % 12 != 0 and 30 % 4 != 0
    assert {v["NQ"] for v in inner.values()} | {v["NQ"] for v in binner.values()} == {2, 4, 8, 16, 24}
    # the group kernels: one block / just over a block of G * C, and the grid-stride pass
    assert sorted(R.cdiv(G * C, 256) for G, C in R.SUM_GC) == [1, 1, 1, 2] and (1, 256) in R.SUM_GC and (1, 257) in R.SUM_GC
    G, P, C = R.BCAST_BIG
    assert G * P * C == 540672 and R.ew_blocks(G * P * C) == 2048 < R.cdiv(G * P * C, 256)
    assert R.POOLED_Q_F - 2048 == 3


def test_dispatch_mirrors_match_the_source():
    """The conditions the mirrors restate are the ones in pool.hip (a changed threshold fails here, not silently in the tables)."""
    src = open(os.path.join(CSRC, "pool.hip")).read()
    for needle in ("const size_t tile = ((size_t)P * C + P) * sizeof(float);",
                   "const bool vec_ok = (C % 4) == 0 && ((((uintptr_t)X) | ((uintptr_t)w) | ((uintptr_t)vec)) & 15) == 0;",
                   "if (vec_ok && P <= 32 && C <= 1024) {", "if (P <= 20) hipLaunchKernelGGL((attn_pool_fwd_reg_kernel<20>)",
                   "else hipLaunchKernelGGL((attn_pool_fwd_reg_kernel<32>)", "if (vec_ok && tile <= 96 * 1024) {",
                   "if (int e = mmego_allow_lds<attn_pool_fwd_lds_kernel>(tile)) return e;",
                   "while (TPP * 2 * P <= 256 && TPP * 2 * P <= 1024 && (C % (TPP * 2)) == 0) TPP *= 2;",
                   "const bool wide = P * TPP <= 1024 && P <= 1024;", "const int PG = (C <= 128 && (256 % C) == 0) ? 256 / C : 1;",
                   "const bool wl = C <= 1024;", "c = c0 + (c >= len ? c % len : c);",
                   "const int nq = (n4 + 255) / 256;", "if (nq <= 2) tile_to_lds<2>(src, dst, n4, tid);",
                   "else if (nq <= 4) tile_to_lds<4>(src, dst, n4, tid);", "else if (nq <= 8) tile_to_lds<8>(src, dst, n4, tid);",
                   "else if (nq <= 16) tile_to_lds<16>(src, dst, n4, tid);", "else tile_to_lds<24>(src, dst, n4, tid);",
                   "const size_t tile = ((size_t)P * C + 2 * P + (size_t)PG * C) * sizeof(float);",
                   "if ((C % 4) == 0 && (256 % TCc) == 0 && tile <= 64 * 1024 && (((uintptr_t)X) & 15) == 0) {",
                   "if (int e = mmego_allow_lds<attn_pool_bwd_lds_kernel>(tile)) return e;",
                   "while (TPP * 2 * P <= 256 && (C % (TPP * 2)) == 0) TPP *= 2;", "if (P * TPP <= 1024) {", "const bool dl = C <= 1024;",
                   "const int TCc = C < 256 ? C : 256, PG = 256 / TCc;", "__shared__ float dvs[1024];", "__shared__ float ps[1024];",
                   "__shared__ float wsh[1024];", "__shared__ __attribute__((aligned(16))) float part[1024];",
                   "const unsigned grid = (unsigned)(F < 2048 ? F : 2048);", "return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));",
                   "const int nb1 = cdiv(G * C1, 256), nb2 = cdiv(G * C2, 256);"):
        assert needle in src, needle
    assert src.count("const int TCc = C < 256 ? C : 256, PG = 256 / TCc;") == 2          # the kernel's split and the launcher's tile size
    assert R.BWD_STATIC_LDS == R.FWD_STATIC_LDS == 4 * (1024 + 1024 + 8)
    # every launch of pool.hip with dynamic LDS that can pass 64 KB with its static arrays goes through mmego_allow_lds
    assert src.count("mmego_allow_lds<") == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# the bounds are tight enough to catch a wrong kernel: mutants of the EMULATION, one per kernel family
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mutated_emulations_are_far_outside_the_bounds():
    """Each must push a ratio past 100 in the comparison named while the true emulation stays under 1.  (Run on the emulation: a kernel
    made wrong on purpose never runs on a GPU.)"""
    far, true = {}, {}
    I = R.pool_inputs(3, 33, 64)
    ref = R.attn_pool_fwd(I["X"], I["w"], I["b"])
    # 1. the softmax normalised by a sum that misses the last point's term
    far["attn_pool_fwd attn"] = R.worst_ratio(R.emu_attn_pool_fwd(I["X"], I["w"], I["b"], mutant="wrong sum")[0], *ref["attn"])[0]
    true["attn_pool_fwd attn"] = R.worst_ratio(R.emu_attn_pool_fwd(I["X"], I["w"], I["b"])[0], *ref["attn"])[0]
    # 2. ds without the - dot term;  3. dX with w and dvec swapped
    J = R.pool_inputs(3, 33, 16)
    attn = R.attn_pool_fwd(J["X"], J["w"], J["b"])["attn"][0].float()
    back = R.attn_pool_bwd(J["X"], J["w"], attn, J["dvec"])
    ok = R.emu_attn_pool_bwd(J["X"], J["w"], attn, J["dvec"])
    far["attn_pool_bwd pdb"] = R.worst_ratio(R.emu_attn_pool_bwd(J["X"], J["w"], attn, J["dvec"], mutant="no dot")[2], *back["pdb"])[0]
    far["attn_pool_bwd dX"] = R.worst_ratio(R.emu_attn_pool_bwd(J["X"], J["w"], attn, J["dvec"], mutant="swapped")[0], *back["dX"])[0]
    true["attn_pool_bwd pdb"], true["attn_pool_bwd dX"] = R.worst_ratio(ok[2], *back["pdb"])[0], R.worst_ratio(ok[0], *back["dX"])[0]
    # 4. cross attention: dS without scale
    Kx = R.cross_inputs(3)
    Pg = R.cross_fwd(Kx["Q"], Kx["K"], Kx["V"], 0.125)["P"][0].float()
    cb = R.cross_bwd(Kx["Q"], Kx["K"], Kx["V"], Pg, Kx["dO"], 0.125)
    far["cross_attn_bwd dQ"] = R.worst_ratio(R.emu_cross_bwd(Kx["Q"], Kx["K"], Kx["V"], Pg, Kx["dO"], 0.125, mutant="no scale")[0], *cb["dQ"])[0]
    true["cross_attn_bwd dQ"] = R.worst_ratio(R.emu_cross_bwd(Kx["Q"], Kx["K"], Kx["V"], Pg, Kx["dO"], 0.125)[0], *cb["dQ"])[0]
    # 5. a group sum that drops row P - 1 when P % 8 == 1 (the unrolled loop's last, lone row)
    X, _ = R.sum_inputs(3, 9, 5)
    far["group_sum"] = R.worst_ratio(R.emu_rows_sum(X, 1.0, mutant="drops last"), *R.group_sum(X, 1.0))[0]
    true["group_sum"] = R.worst_ratio(R.emu_rows_sum(X, 1.0), *R.group_sum(X, 1.0))[0]
    print("\n".join("MUTANT %-24s ratio %.3g (true emulation %.3g)" % (k, v, true[k]) for k, v in far.items()))
    assert all(v > 100.0 for v in far.values()), far
    assert all(v <= 1.0 for v in true.values()), true
