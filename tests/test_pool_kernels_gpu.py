"""GPU: the pooling and attention kernels of csrc/pool.hip, each on its own through the C ABI, against float64 (tests/pool_ref.py):
attention pooling forward (register, LDS and plain kernels) and backward (LDS and plain), the group sums and broadcasts and their
two-problem forms, cross attention forward (matrix-pipe and scalar kernels), its pooled forms, its backward, and mmego_graph_dA.

Method of tests/test_lstm_kernels_gpu.py and tests/test_gcn_train_gpu.py (their helpers are used): every reference is plain float64 torch
on the CPU computed from the fp32 values the kernel read; |out - ref| <= MARGIN * bound elementwise with the a-priori bounds pool_ref.py
derives (MARGIN = 4); no element is left out; operands lie in buffers with NaN around them, every output is surrounded by a sentinel that
must survive; the LDS kernels run behind a launch that left NaN in every compute unit's LDS.  Every attention case holds ordinary rows,
rows with one score ahead by 30 and by 200 (weights exactly 0 and 1), tied rows (attn == 1 / P), rows with all scores near -100, and runs
with b given and with b == NULL.  Where the source fixes a summation order and the result can be seen, the test asks for the bits of the
fp32 emulation: the group sums, the pooled cross attention's sum over the queries, the weighted sum of the attention pooling restated
from the kernel's OWN stored weights, and pdb, pdw and dX of both attention-pooling backward kernels (no expf stands between their
inputs and outputs).  NOTES.md ("Float64 tests of the pooling and attention kernels") holds the measured error /
bound ratios; tests/test_pool_ref_cpu.py pins which kernel and which inner branch each case reaches."""
import pytest
import torch

import gcn_train_ref as GR
import pool_ref as R
import test_lstm_kernels_gpu as L
from test_lstm_kernels_gpu import Wide, same_bits
from test_gcn_train_gpu import Out, d_vec, d_mat, refused, call, poison_lds, NAN

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
            print("RATIO %-26s %-14s %.4g" % (k, o, r))


def check(kernel, name, out, ref, bound, note=""):
    """test_lstm_kernels_gpu.check, with the ratio kept in this file's table.  (That check records into its own module's RATIOS; the
    entry is taken out again at once, and the kernel names used here -- pool_*, cross_*, group_*, graph_dA -- are disjoint from the
    LSTM file's, so neither table ever shows the other's rows.)"""
    try:
        L.check(kernel, name, out, ref, bound, note)
    finally:
        RATIOS[(kernel, name)] = max(RATIOS.get((kernel, name), 0.0), L.RATIOS.pop((kernel, name), 0.0))


def short(kernel):
    return kernel.replace("_kernel", "").replace("attn_pool_", "pool_")


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_attn_pool_forward
# ---------------------------------------------------------------------------------------------------------------------------------
def run_pool_fwd(dev, I, off=0):
    """-> (attn [G][P], vec [G][C]) on the CPU; guards checked."""
    G, P, C = I["X"].shape
    X = Wide(dev, G * P, C, C, fill=NAN, src=I["X"], lead=off)
    w, b = d_vec(dev, I["w"]), None if I["b"] is None else d_vec(dev, torch.tensor([I["b"]]))
    vec, attn = Out(dev, G, C, strided=False), Out(dev, G, P, strided=False)
    if R.fwd_kernel(P, C, not off) == "attn_pool_fwd_lds_kernel":
        poison_lds(dev)
    call("attn_pool_forward", X.view, w, b, G, P, C, vec.view, attn.view)
    assert vec.guards_intact() and attn.guards_intact() and X.guards_intact(), ("guards", G, P, C, off)
    return attn.cpu(), vec.cpu()


def check_pool_fwd(dev, case, shift):
    P, C, G, off, kernel = case
    assert R.fwd_kernel(P, C, not off) == kernel
    I = R.pool_inputs(G, P, C, shift)
    ref = R.attn_pool_fwd(I["X"], I["w"], I["b"])
    a, vec = run_pool_fwd(dev, I, off)
    note, k = (P, C, G, off, shift, kernel), short(kernel)
    check(k, "attn", a, *ref["attn"], note)
    check(k, "vec", vec, *ref["vec"], note)
    tied, sat = I["kinds"] == 3, I["kinds"] == 2
    assert bool((a[tied] == torch.tensor(1.0 / P).float()).all()), ("tied rows: attn == 1 / P", note)
    if P > 1:
        assert bool(((a[sat] == 0) | (a[sat] == 1)).all()) and bool((a[sat].sum(-1) == 1).all()), ("saturated rows: weights 0 and 1", note)
    # the weighted sum is fixed-order: from the kernel's own stored weights it has the bits of the emulation
    PG = R.fwd_lds_inner(P, C)["PG"] if kernel == "attn_pool_fwd_lds_kernel" else 1
    assert same_bits(vec, R.emu_colsum(I["X"], a, PG)), ("vec is not the fixed-order sum of x_p attn_p", note)
    return I, a, vec, ref


@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: "-".join(str(v) for v in c[:4]))
def test_attn_pool_forward(dev, case):
    P, C, G, off, kernel = case
    for shift in R.shifts(G):
        I, a, vec, ref = check_pool_fwd(dev, case, shift)
        if shift == 0:      # a second launch has the same bits (no order depends on scheduling)
            a2, vec2 = run_pool_fwd(dev, I, off)
            assert same_bits(a, a2) and same_bits(vec, vec2), ("two launches differ", case)


def test_attn_pool_forward_forms_agree(dev):
    """(20, 64) reaches the register kernel aligned and the plain kernel with X one float past alignment; (33, 64) the LDS kernel and the
    plain one: the same inputs through both, each within its bound of float64 and so within two of each other."""
    for P, C, first in ((20, 64, "attn_pool_fwd_reg_kernel<20>"), (33, 64, "attn_pool_fwd_lds_kernel")):
        for shift in R.shifts(3):
            I = R.pool_inputs(3, P, C, shift)
            assert R.fwd_kernel(P, C, True) == first and R.fwd_kernel(P, C, False) == "attn_pool_fwd_kernel"
            ref = R.attn_pool_fwd(I["X"], I["w"], I["b"])
            (a0, v0), (a1, v1) = run_pool_fwd(dev, I, 0), run_pool_fwd(dev, I, 1)
            check("pool_fwd forms", "attn", a1, a0.double(), 2 * ref["attn"][1], (P, C, shift))
            check("pool_fwd forms", "vec", v1, v0.double(), 2 * ref["vec"][1], (P, C, shift))
            check("pool_fwd", "attn", a1, *ref["attn"], (P, C, shift, "misaligned"))
            check("pool_fwd", "vec", v1, *ref["vec"], (P, C, shift, "misaligned"))


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_attn_pool_backward
# ---------------------------------------------------------------------------------------------------------------------------------
def run_pool_bwd(dev, I, attn, off=0):
    G, P, C = I["X"].shape
    X = Wide(dev, G * P, C, C, fill=NAN, src=I["X"], lead=off)
    ops = [d_vec(dev, I["w"]), d_vec(dev, attn), d_vec(dev, I["dvec"])]
    dX, pdw, pdb = Out(dev, G * P, C, strided=False), Out(dev, G, C, strided=False), Out(dev, 1, G, strided=False)
    if R.bwd_kernel(P, C, not off) == "attn_pool_bwd_lds_kernel":
        poison_lds(dev)
    call("attn_pool_backward", X.view, ops[0], ops[1], ops[2], G, P, C, dX.view, pdw.view, pdb.view)
    assert dX.guards_intact() and pdw.guards_intact() and pdb.guards_intact() and X.guards_intact(), ("guards", G, P, C, off)
    return dX.cpu().view(G, P, C), pdw.cpu(), pdb.cpu()[0]


@pytest.mark.parametrize("case", R.BWD_CASES, ids=lambda c: "-".join(str(v) for v in c[:4]))
def test_attn_pool_backward(dev, case):
    """attn is the float64 softmax of the case's inputs rounded to fp32 (exact zeros, ones and 1 / P among it).  (120, 128): 63,424
    bytes of tile and 8,224 of static arrays, 71,648 in all -- the launch that needs the raised dynamic-LDS limit."""
    P, C, G, off, kernel = case
    assert R.bwd_kernel(P, C, not off) == kernel
    for shift in R.shifts(G):
        I = R.pool_inputs(G, P, C, shift)
        attn = R.attn_pool_fwd(I["X"], I["w"], I["b"])["attn"][0].float()
        ref = R.attn_pool_bwd(I["X"], I["w"], attn, I["dvec"])
        got = run_pool_bwd(dev, I, attn, off)
        note, k = (P, C, G, off, shift, kernel), short(kernel)
        for name, o in zip(("dX", "pdw", "pdb"), got):
            check(k, name, o, *ref[name], note)
        # no expf between the inputs and the outputs, every order fixed by the source ("partials summed in fixed order", the workgroup
        # reductions, the PG row groups): pdb and pdw have the bits of the emulation.  dX = attn dvec + ds w is one product and one fma;
        # which product is fused the source leaves to the compiler: either form, the same one for the whole tensor.
        emu = [R.emu_attn_pool_bwd(I["X"], I["w"], attn, I["dvec"], kernel, dx_form=f) for f in (0, 1)]
        assert same_bits(got[2], emu[0][2]), ("pdb is not the fixed-order emulation's", note)
        assert same_bits(got[1], emu[0][1]), ("pdw is not the fixed-order emulation's", note)
        assert same_bits(got[0], emu[0][0]) or same_bits(got[0], emu[1][0]), ("dX is neither fused form of the emulation", note)
        if shift == 0:
            again = run_pool_bwd(dev, I, attn, off)
            assert all(same_bits(x, y) for x, y in zip(got, again)), ("two launches differ", case)
            # one non-zero weight of 0.5 per group: pdb = da / 4 exactly -- one row's da, TPP partials and their order, seen from outside
            half, ps = R.half_attn(G, P)
            hgot = run_pool_bwd(dev, I, half, off)
            da, _ = R.emu_da(I["X"], I["dvec"], kernel)
            assert same_bits(hgot[2] * 4.0, da[torch.arange(G), ps]), ("pdb of a one-entry attn is not that row's da / 4", note)
            hemu = R.emu_attn_pool_bwd(I["X"], I["w"], half, I["dvec"], kernel)
            assert same_bits(hgot[2], hemu[2]) and same_bits(hgot[1], hemu[1]), ("one-entry attn", note)
            href = R.attn_pool_bwd(I["X"], I["w"], half, I["dvec"])
            for name, o in zip(("dX", "pdw", "pdb"), hgot):
                check(k, name, o, *href[name], note + ("half",))
        if (P, C, off) == (128, 64, 1):     # the same inputs through the LDS kernel
            other = run_pool_bwd(dev, I, attn, 0)
            for name, o, o2 in zip(("dX", "pdw", "pdb"), got, other):
                check("pool_bwd forms", name, o, o2.double(), 2 * ref[name][1], note)


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_cross_attn_forward, _pooled, _pooled_q
# ---------------------------------------------------------------------------------------------------------------------------------
def kv_buffer(dev, I, ldkv):
    F = I["K"].shape[0]
    return Wide(dev, F * R.NK, 128, ldkv, fill=NAN, src=torch.cat((I["K"], I["V"]), -1))


def run_cross_fwd(dev, I, aligned):
    """-> (P [F][64][15], O [F][64][64]) through cross_attn_fwd_mfma_kernel<false, false> (aligned) or cross_attn_fwd_kernel (Q one float
    past alignment, ldkv and ldo odd)."""
    F = I["K"].shape[0]
    ldkv, ldo = (132, 128) if aligned else (131, 67)
    Q = Wide(dev, F * R.NQ, 64, 64, fill=NAN, src=I["Q"], lead=0 if aligned else 1)
    KV = kv_buffer(dev, I, ldkv)
    O, Pm = Wide(dev, F * R.NQ, 64, ldo, col=ldo - 64 if aligned else 0), Out(dev, F * R.NQ, R.NK, strided=False)
    call("cross_attn_forward", Q.view, KV.view[:, :64], KV.view[:, 64:], F, I["scale"], O.view, ldo, Pm.view, ldkv)
    assert O.guards_intact() and Pm.guards_intact() and KV.guards_intact(), ("guards", F, aligned)
    return Pm.cpu().view(F, R.NQ, R.NK), O.cpu().view(F, R.NQ, 64)


def check_kinds(I, Pm, note):
    """The rows the masked 16th slot and the saturated softmax are held to account by."""
    for f, k in enumerate(I["kinds"].tolist()):
        if k in (1, 7):
            assert bool((Pm[f, :, 14] > 0.999).all()), ("key 14 leads: its weight is 1, not one half", f, note)
        if k == 2:
            assert bool((Pm[f, :, 0] > 0.999).all()), (f, note)
        if k in (3, 7):
            assert bool(((Pm[f] == 0) | (Pm[f] == 1)).all()) and bool((Pm[f].sum(-1) == 1).all()), (f, note)
        if k == 4:
            assert bool((Pm[f] == Pm[f, 0, 0]).all()) and abs(float(Pm[f, 0, 0]) - 1.0 / 15) < 1e-7, (f, note)


@pytest.mark.parametrize("F", R.CROSS_F)
def test_cross_attn_forward(dev, F):
    for shift in R.shifts(F, 8):
        I = R.cross_inputs(F, shift)
        ref = R.cross_fwd(I["Q"], I["K"], I["V"], I["scale"])
        got = {}
        for aligned, k in ((True, "cross_fwd_mfma"), (False, "cross_fwd scalar")):
            Pm, O = got[aligned] = run_cross_fwd(dev, I, aligned)
            check(k, "P", Pm, *ref["P"], (F, shift))
            check(k, "O", O, *ref["O"], (F, shift))
            check_kinds(I, Pm, (F, shift, k))
        check("cross_fwd forms", "P", got[True][0], got[False][0].double(), 2 * ref["P"][1], (F, shift))
        check("cross_fwd forms", "O", got[True][1], got[False][1].double(), 2 * ref["O"][1], (F, shift))


@pytest.mark.parametrize("F", R.CROSS_F)
def test_cross_attn_forward_pooled(dev, F):
    """Against float64, and bit for bit the row-order sum of the unpooled kernel's O: by the emulation and by mmego_group_sum2."""
    for shift in R.shifts(F, 8):
        I = R.cross_inputs(F, shift)
        ref = R.cross_fwd(I["Q"], I["K"], I["V"], I["scale"])
        Q, KV = d_vec(dev, I["Q"]), kv_buffer(dev, I, 132)
        osum = Wide(dev, F, 64, 192, col=64)
        call("cross_attn_forward_pooled", Q, KV.view[:, :64], KV.view[:, 64:], F, I["scale"], osum.view, 192, 132)
        assert osum.guards_intact(), ("sentinel columns of osum", F, shift)
        check("cross_fwd_mfma pooled", "osum", osum.cpu(), *ref["osum"], (F, shift))
        _, O = run_cross_fwd(dev, I, True)
        assert same_bits(osum.cpu(), R.emu_rows_sum(O, 1.0)), ("osum is not the row-order sum of the unpooled O", F, shift)
        two = Wide(dev, F, 64, 192, col=64)
        kvs = Wide(dev, F, 64, 68)
        call("group_sum2", F, O.to(dev).contiguous(), 64, 64, 1.0, two.view, 192, I["K"].to(dev).contiguous(), R.NK, 64, 1.0, kvs.view, 68)
        assert same_bits(osum.cpu(), two.cpu()) and two.guards_intact() and kvs.guards_intact(), ("the order of group_sum2", F, shift)
        assert same_bits(kvs.cpu(), R.emu_rows_sum(I["K"], 1.0))


def test_cross_attn_forward_pooled_q_second_round(dev):
    """F = 2051: the persistent launch has 2048 workgroups, workgroups 0..2 walk on to frames 2048..2050 (osh reused behind the trailing
    barrier, the workgroup's copy of Wq reused).  Every frame is checked, frames 0..2 and 2048..2050 among them, all eight row kinds."""
    F = R.POOLED_Q_F
    I = R.cross_inputs(F, proj=True)
    q, e_q = R.query_proj(I["X"], I["Wq"], I["bq"])
    ref = R.cross_fwd(q, I["K"], I["V"], I["scale"], e_q)
    X = Wide(dev, F * R.NQ, 64, 68, fill=NAN, src=I["X"])
    Wq, bq, KV = d_vec(dev, I["Wq"]), d_vec(dev, I["bq"]), kv_buffer(dev, I, 132)
    osum = Wide(dev, F, 64, 192, col=64)
    call("cross_attn_forward_pooled_q", X.view, 68, Wq, bq, KV.view[:, :64], KV.view[:, 64:], F, I["scale"], osum.view, 192, 132)
    assert osum.guards_intact(), "sentinel columns of osum"
    got = osum.cpu()
    check("cross_fwd_mfma pooled_q", "osum", got, *ref["osum"], F)
    for f in (0, 1, 2, 2047, 2048, 2049, 2050):
        assert R.worst_ratio(got[f], ref["osum"][0][f], ref["osum"][1][f])[0] <= R.MARGIN, f
    assert {int(I["kinds"][f]) for f in (2048, 2049, 2050)} == {0, 1, 2}        # key 14 ahead and key 0 ahead in the second round
    # the same frames one per workgroup (F = 3: no second round) have the same bits
    J = {k: (v[2048:].contiguous() if k in ("X", "K", "V") else v) for k, v in I.items()}
    X3, KV3, o3 = Wide(dev, 3 * R.NQ, 64, 68, fill=NAN, src=J["X"]), kv_buffer(dev, J, 132), Wide(dev, 3, 64, 192, col=64)
    call("cross_attn_forward_pooled_q", X3.view, 68, Wq, bq, KV3.view[:, :64], KV3.view[:, 64:], 3, I["scale"], o3.view, 192, 132)
    assert same_bits(o3.cpu(), got[2048:]) and o3.guards_intact()


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_cross_attn_backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", R.CROSS_F)
def test_cross_attn_backward(dev, F):
    """dO the right half of a NaN-padded [.., 128] buffer, K | V one [.., 128] buffer, dK | dV the halves of one sentinel buffer; P the
    float64 softmax rounded to fp32: ordinary, one-hot and exactly-zero entries."""
    for shift in R.shifts(F, 8):
        I = R.cross_inputs(F, shift)
        Pg = R.cross_fwd(I["Q"], I["K"], I["V"], I["scale"])["P"][0].float()
        if {3, 7} & set(I["kinds"].tolist()):
            assert bool((Pg == 0).any()) and bool((Pg == 1).any())
        Q, Pd, KV = d_vec(dev, I["Q"]), d_vec(dev, Pg), kv_buffer(dev, I, 128)
        dO = Wide(dev, F * R.NQ, 64, 128, col=64, fill=NAN, src=I["dO"])
        for scale in (0.125, 1.0):
            ref = R.cross_bwd(I["Q"], I["K"], I["V"], Pg, I["dO"], scale)
            dQ, dKV = Out(dev, F * R.NQ, 64, strided=False), Wide(dev, F * R.NK, 128, 128)
            call("cross_attn_backward", Q, KV.view[:, :64], KV.view[:, 64:], Pd, dO.view, 128, F, scale, dQ.view, dKV.view[:, :64],
                 dKV.view[:, 64:], 128)
            assert dQ.guards_intact() and dKV.guards_intact(), ("guards", F, shift)
            g = dKV.cpu().view(F, R.NK, 128)
            check("cross_bwd", "dQ", dQ.cpu().view(F, R.NQ, 64), *ref["dQ"], (F, shift, scale))
            check("cross_bwd", "dK", g[:, :, :64], *ref["dK"], (F, shift, scale))
            check("cross_bwd", "dV", g[:, :, 64:], *ref["dV"], (F, shift, scale))


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_group_sum, _sum2, _bcast, _bcast2
# ---------------------------------------------------------------------------------------------------------------------------------
def test_group_sum(dev):
    """P across the 8-row unrolled loop's edges, G * C under, at and over one block; the bits of the fp32 row-order sum."""
    for P in R.SUM_P:
        for G, C in R.SUM_GC:
            X, _ = R.sum_inputs(G, P, C)
            Y = Wide(dev, G, C, C + 3)
            call("group_sum", d_vec(dev, X), G, P, C, 1.0 / P, Y.view, C + 3)
            assert Y.guards_intact(), (P, G, C)
            check("group_sum", "Y", Y.cpu(), *R.group_sum(X, float(torch.tensor(1.0 / P).float())), (P, G, C))
            assert same_bits(Y.cpu(), R.emu_rows_sum(X, 1.0 / P)), ("summed in row order", P, G, C)


def test_group_sum2(dev):
    """Two problems of different (P, C, scale, ld) per launch; the second problem's first element when the first one fills its last block
    (G * C1 = 256) and when it spills one element into another (257)."""
    for i, P1 in enumerate(R.SUM_P):
        for G, C1 in R.SUM_GC:
            P2, C2 = R.SUM_P[(i + 2) % len(R.SUM_P)], 7 if C1 != 5 else 64
            X1, _ = R.sum_inputs(G, P1, C1, 1)
            X2, _ = R.sum_inputs(G, P2, C2, 2)
            Y1, Y2 = Wide(dev, G, C1, C1 + 3), Wide(dev, G, C2, C2 + 1)
            call("group_sum2", G, d_vec(dev, X1), P1, C1, 1.0 / P1, Y1.view, C1 + 3, d_vec(dev, X2), P2, C2, 0.5, Y2.view, C2 + 1)
            assert Y1.guards_intact() and Y2.guards_intact(), (P1, G, C1)
            check("group_sum2", "Y1", Y1.cpu(), *R.group_sum(X1, float(torch.tensor(1.0 / P1).float())), (P1, G, C1))
            check("group_sum2", "Y2", Y2.cpu(), *R.group_sum(X2, 0.5), (P2, G, C2))
            assert same_bits(Y1.cpu(), R.emu_rows_sum(X1, 1.0 / P1)) and same_bits(Y2.cpu(), R.emu_rows_sum(X2, 0.5)), (P1, G, C1)
            assert same_bits(Y2.cpu()[:1, :1], R.emu_rows_sum(X2, 0.5)[:1, :1]) and same_bits(Y1.cpu()[-1:, -1:], R.emu_rows_sum(X1, 1.0 / P1)[-1:, -1:])


def bcast_shapes():
    return [(G, P, C) for P in R.SUM_P for G, C in R.SUM_GC] + [R.BCAST_BIG]


def test_group_bcast(dev):
    """accumulate 0 and 1, lddy > C; the last shape has 540,672 elements: the 2048 blocks take a second pass."""
    for G, P, C in bcast_shapes():
        X0, dY = R.sum_inputs(G, P, C, 3)
        dYd = Wide(dev, G, C, C + 3, fill=NAN, src=dY)
        for acc in (0, 1):
            dX = Out(dev, G * P, C, strided=False)
            dX.view.copy_(X0.view(G * P, C))
            call("group_bcast", dYd.view, C + 3, G, P, C, 0.75, dX.view, acc)
            assert dX.guards_intact(), (G, P, C, acc)
            check("group_bcast", "dX acc%d" % acc, dX.cpu().view(G, P, C), *R.group_bcast(dY, P, 0.75, X0 if acc else None), (G, P, C))
            if not acc:
                assert same_bits(dX.cpu().view(G, P, C), R.emu_group_bcast(dY, P, 0.75))


def test_group_bcast2(dev):
    shapes = bcast_shapes()
    for i, (G, P1, C1) in enumerate(shapes):
        P2, C2 = (shapes[(i + 5) % len(shapes)][1], 7) if (G, P1, C1) != R.BCAST_BIG else (15, 64)
        _, dY1 = R.sum_inputs(G, P1, C1, 4)
        _, dY2 = R.sum_inputs(G, P2, C2, 5)
        d1, d2 = Wide(dev, G, C1, C1 + 3, fill=NAN, src=dY1), Wide(dev, G, C2, C2 + 1, fill=NAN, src=dY2)
        o1, o2 = Out(dev, G * P1, C1, strided=False), Out(dev, G * P2, C2, strided=False)
        call("group_bcast2", G, d1.view, C1 + 3, P1, C1, 1.0 / P1, o1.view, d2.view, C2 + 1, P2, C2, 0.5, o2.view)
        assert o1.guards_intact() and o2.guards_intact(), (G, P1, C1)
        s1 = float(torch.tensor(1.0 / P1).float())
        check("group_bcast2", "dX1", o1.cpu().view(G, P1, C1), *R.group_bcast(dY1, P1, s1), (G, P1, C1))
        check("group_bcast2", "dX2", o2.cpu().view(G, P2, C2), *R.group_bcast(dY2, P2, 0.5), (G, P2, C2))
        assert same_bits(o1.cpu().view(G, P1, C1), R.emu_group_bcast(dY1, P1, 1.0 / P1)) and same_bits(o2.cpu().view(G, P2, C2), R.emu_group_bcast(dY2, P2, 0.5))


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_graph_dA (the unfused entry nets.py still calls), against gcn_train_ref.graph_dA as it stands: dY is an input here, exact, so
# the reference's allowance for the roundings the fused kernel spends on forming dY is slack, not error
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K", ((15, 2), (7, 3), (1, 1), (15, 1)))
def test_graph_dA(dev, V, K):
    from mmego_amd import hip
    for G in (1, 2, 3, 37):
        for C in (16, 64):
            g = R.gen_for(74, G, V, K, C)
            rows, sliced = G * V, bool((G + C // 16 + K) & 1)
            Z, dY = torch.randn(rows, K * C, generator=g) * 0.9, torch.randn(rows, C, generator=g)
            A, imp = torch.randn(K, V, V, generator=g) * 0.4, torch.rand(K, V, V, generator=g) + 0.5
            Zd, ldz = d_mat(dev, Z, sliced)
            nblk = hip.graph_dA_nblk(G)
            assert nblk == (G + 1) // 2
            o_p, o_dz = Out(dev, nblk, K * V * V, strided=False, guard=2), Out(dev, rows, K * C, sliced)
            poison_lds(dev)
            call("graph_dA", Zd, d_vec(dev, dY), G, V, K, C, o_p.view, d_vec(dev, A), d_vec(dev, imp), o_dz.view, ldz, o_dz.ld)
            ref = GR.graph_dA(Z, dY.double(), dY.double().abs(), A, imp, G, V, K, C)
            note = (G, V, K, C, sliced)
            check("graph_dA", "dZ", o_dz.cpu(), *ref["dZ"], note)
            check("graph_dA", "partial", o_p.cpu().view(nblk, K, V, V), *ref["partial"], note)
            assert o_p.guards_intact() and o_dz.guards_intact(), note
            o_q = Out(dev, nblk, K * V * V, strided=False, guard=2)          # without dZ: the same partials
            call("graph_dA", Zd, d_vec(dev, dY), G, V, K, C, o_q.view, None, None, None, ldz, 0)
            assert same_bits(o_q.cpu(), o_p.cpu()) and o_q.guards_intact(), note


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: every MMEGO_REQUIRE of the entry points above
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
    off = t[1:]           # one float past a 16-byte address
    each_refused("attn_pool_forward", [t, t, t, 3, 7, 36, t, t], (0, 1, 6, 7), ((3, 0), (4, 0), (5, 0), (4, 8193), (3, -1)))
    each_refused("attn_pool_backward", [t, t, t, t, 3, 7, 36, t, t, t], (0, 1, 2, 3, 7, 8, 9), ((4, 0), (5, 0), (6, 0), (5, 8193)))
    each_refused("group_sum", [t, 3, 7, 5, 1.0, t, 5], (0, 5), ((1, 0), (2, 0), (3, 0)))
    each_refused("group_sum2", [3, t, 7, 5, 1.0, t, 5, t, 9, 7, 1.0, t, 7], (1, 5, 7, 11), ((0, 0), (2, 0), (3, 0), (8, 0), (9, 0)))
    each_refused("group_bcast", [t, 5, 3, 7, 5, 1.0, t, 0], (0, 6), ((2, 0), (3, 0), (4, 0)))
    each_refused("group_bcast2", [3, t, 5, 7, 5, 1.0, t, t, 7, 9, 7, 1.0, t], (1, 6, 7, 12), ((0, 0), (3, 0), (4, 0), (9, 0), (10, 0)))
    each_refused("cross_attn_forward", [t, t, t, 1, 0.125, t, 64, t, 64], (0, 1, 2, 5, 7), ((3, 0), (8, 63)))
    each_refused("cross_attn_forward_pooled", [t, t, t, 1, 0.125, t, 64, 64], (0, 1, 2, 5),
                 ((3, 0), (7, 63), (6, 63), (0, off), (1, off), (2, off), (7, 65), (7, 66)))
    each_refused("cross_attn_forward_pooled_q", [t, 64, t, t, t, t, 1, 0.125, t, 64, 64], (0, 2, 3, 4, 5, 8),
                 ((6, 0), (10, 63), (9, 63), (1, 63), (0, off), (2, off), (3, off), (4, off), (5, off), (10, 65), (1, 65), (1, 66)))
    each_refused("cross_attn_backward", [t, t, t, t, t, 64, 1, 0.125, t, t, t, 64], (0, 1, 2, 3, 4, 8, 9, 10), ((6, 0), (11, 63)))
    each_refused("graph_dA", [t, t, 2, 15, 2, 16, t, t, t, t, 32, 32], (0, 1, 6), ((2, 0), (3, 0), (4, 0), (5, 0), (4, 3), (10, 31), (11, 31), (7, None), (8, None)))
    refused("graph_dA", t, t, 2, 15, 2, 512, t, None, None, None, 1024, 0)          # more than 64 KB of LDS
    assert bool((t == 0).all())
