"""GPU: the fused ST-GCN training kernels of csrc/gcn_fused.hip and the record-carrying temporal convolutions of csrc/gcn.hip, each on its
own through the C ABI, against float64 (tests/gcn_train_ref.py).

Every reference is plain float64 torch on the CPU computed from the fp32 values the kernel read.  Where a ReLU decision is one
fmaf(y - mean, a, b) > 0 (graph_dA_fused, the bw_rec epilogues) the mask is the kernel's own by the sign identity of
tests/test_mlp_train_gpu.py; where the mask is an input tensor (gcn_bn_bwd_*) it is an input; max(t, 0) outputs are continuous and need
none.  No element is left out of any comparison.

Tolerances are a-priori fp32 rounding bounds, |out - ref| <= MARGIN * bound elementwise (gcn_train_ref.py lists the forms; MARGIN = 4 is
tests/test_mlp_train_gpu.py's).  Outputs a kernel derives from another output of its own (the records of Z / Y / the convolution output,
the rows activated with the state finalized in the prologue) start from the kernel's own fp32 values, with every magnitude inside the
bound taken from the float64 reference of the first output.  NOTES.md ("Float64 tests of the fused ST-GCN training kernels") holds the
measured error / bound ratios.

Operands whose entry point takes a stride run dense and as a column slice of a wider buffer with NaN around it (16-byte bases and
ld % 4 == 0 where the entry point demands them); every output has guard rows, guard columns and guard records pre-filled with a sentinel
that must survive.  test_shape_rules pins why each shape is the case it claims to be."""
import pytest
import torch

import gcn_train_ref as R
from gcn_train_ref import U32, U64, MARGIN, EPS, MOM, CACT

pytestmark = pytest.mark.gpu

SENT = 7777.0
GUARD = 8
NAN = float("nan")
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
            print("RATIO %-22s %-22s %.4g" % (k, o, r))


def call(name, *args):
    from mmego_amd import hip
    hip.call(name, *args)


def refused(name, *args):
    """The entry point returns MMEGO_EBADARG (no launch)."""
    with pytest.raises(RuntimeError, match="bad argument"):
        call(name, *args)


# ---------------------------------------------------------------------------------------------------------------------------------
# device buffers
# ---------------------------------------------------------------------------------------------------------------------------------
def d_mat(dev, t, sliced, al=True):
    """[rows][C] operand -> (device view, ld).  sliced: columns 0..C-1 of a wider buffer, NaN everywhere else; al: 16-byte base and
    ld % 4 == 0 (C % 4 == 0), else a base one float past an aligned address and ld = C + 3."""
    rows, C = t.shape
    if not sliced:
        return t.to(dev).contiguous(), C
    ex, off = (4, 4) if al else (3, 1)
    ld = C + ex
    buf = torch.full((off + rows * ld + ex,), NAN, dtype=t.dtype, device=dev)
    v = buf[off:off + rows * ld].view(rows, ld)[:, :C]
    v.copy_(t)
    return v, ld


def d_vec(dev, t):
    """A contiguous operand (weights, state, records): 16-byte aligned, NaN behind it."""
    flat = t.contiguous().view(-1)
    buf = torch.full((flat.numel() + 4,), NAN, dtype=t.dtype, device=dev)
    buf[:flat.numel()].copy_(flat)
    return buf[:flat.numel()]


def d_rec(dev, rec):
    """Records [nrec][C][2] with two NaN records behind the last (a record read past nrec poisons the result)."""
    nrec, C, _ = rec.shape
    full = torch.full((nrec + 2, C, 2), NAN, dtype=torch.float32)
    full[:nrec] = rec
    return full.to(dev)


class Out:
    """An output [rows][C] with guard rows (and, sliced, guard columns) pre-filled with the sentinel.  strided=False: an output the ABI
    takes without a leading dimension (records: the guard rows are guard records, the one behind the last included)."""

    def __init__(self, dev, rows, C, sliced=False, al=True, strided=True, guard=GUARD, dtype=torch.float32):
        ex, off = ((4, 4) if al else (3, 1)) if (sliced and strided) else (0, 0)
        self.rows, self.C, self.ld, self.off, self.guard = rows, C, C + ex, off, guard
        self.buf = torch.full((off + (rows + guard) * self.ld,), SENT, dtype=dtype, device=dev)
        self.view = self.buf[off:].view(rows + guard, self.ld)[:rows, :C]

    def cpu(self):
        return self.view.cpu()

    def guards_intact(self):
        b = self.buf.clone()
        b[self.off:].view(self.rows + self.guard, self.ld)[:self.rows, :self.C] = SENT
        return bool((b == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def gen_for(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def randn(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


def rand_bn(g, C):
    """gamma (either sign), beta, running mean, running variance."""
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    return gamma, randn(g, C, scale=0.3), randn(g, C, scale=0.4), torch.rand(C, generator=g) + 0.5


def rand_state(g, C):
    """A sane BatchNorm state [4][C]: mean, invstd > 0, a = gamma invstd (either sign), b."""
    mean, invstd = randn(g, C, scale=0.3), torch.rand(C, generator=g) + 0.5
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    return torch.stack((mean, invstd, gamma * invstd, randn(g, C, scale=0.3)))


class Bn:
    """One BatchNorm whose statistics arrive as records: device copies of its parameters, sentinel-guarded state and running statistics,
    and the MmegoBnRef over them."""

    def __init__(self, dev, g, C, rec, rpr, state=True, running=True):
        from mmego_amd import hip
        self.C, self.rec, self.rpr = C, rec, rpr
        self.gamma, self.beta, self.rm0, self.rv0 = rand_bn(g, C)
        self.o_state = Out(dev, 4, C, strided=False) if state else None
        self.o_rm = Out(dev, 1, C, strided=False) if running else None
        self.o_rv = Out(dev, 1, C, strided=False) if running else None
        if running:
            self.o_rm.view.copy_(self.rm0.view(1, -1))
            self.o_rv.view.copy_(self.rv0.view(1, -1))
        self.keep = [d_vec(dev, self.gamma), d_vec(dev, self.beta), None if rec is None else d_rec(dev, rec)]
        self.ref = hip.BnRef(rec=hip.ptr(self.keep[2]), nrec=0 if rec is None else rec.shape[0], rows_per_rec=rpr, gamma=hip.ptr(self.keep[0]),
                             beta=hip.ptr(self.keep[1]), running_mean=hip.ptr(self.o_rm.view if running else None),
                             running_var=hip.ptr(self.o_rv.view if running else None), momentum=MOM, eps=EPS,
                             state=hip.ptr(self.o_state.view if state else None))

    def check(self, kernel, stats, note):
        """state and running statistics against float64 (stats: gcn_train_ref.stats_*); they started from non-trivial values, so a second
        update (or none) is off by momentum |statistic - old value| -- they were updated exactly once.  -> the kernel's own state."""
        got = None
        if self.o_state is not None:
            got = self.o_state.cpu()
            for q, nm in enumerate(("mean", "invstd", "a", "b")):
                check(kernel, "state." + nm, got[q], stats["state"][0][q], stats["state"][1][q], note)
            assert self.o_state.guards_intact(), (kernel, note)
        if self.o_rm is not None:
            check(kernel, "running_mean", self.o_rm.cpu()[0], *stats["rm"], note)
            check(kernel, "running_var", self.o_rv.cpu()[0], *stats["rv"], note)
            assert self.o_rm.guards_intact() and self.o_rv.guards_intact(), (kernel, note)
        return got


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def check(kernel, name, out, ref, bound, note=""):
    """|out - ref| <= MARGIN * bound elementwise (bound 0: equal), every element; records the largest error / bound ratio."""
    out, ref = out.double().cpu(), ref.double()
    bound = bound.double().expand_as(ref)
    assert out.shape == ref.shape, (kernel, name, out.shape, ref.shape)
    err = (out - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    RATIOS[(kernel, name)] = max(RATIOS.get((kernel, name), 0.0), worst)
    if not worst <= MARGIN:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        bad = int((ratio > MARGIN).sum())
        raise AssertionError("%s %s %s: %d of %d elements off; worst at %s: got %r want %r bound %.3g (ratio %.3g)"
                             % (kernel, name, note, bad, ratio.numel(), idx, float(out[idx]), float(ref[idx]), float(bound[idx]), worst))


def check_records(kernel, name, o_rec, nrec, C, ref, bound, note, summed=False):
    """Records [nrec][C][2] per record (pins the rows a record owns), optionally summed; guard records (the one behind the last) intact."""
    got = o_rec.cpu().view(nrec, C, 2)
    check(kernel, name + ".0", got[:, :, 0], ref[:, :, 0], bound[:, :, 0], note)
    check(kernel, name + ".1", got[:, :, 1], ref[:, :, 1], bound[:, :, 1], note)
    if summed:
        check(kernel, name + " summed", got.double().sum(0), ref.sum(0), bound.sum(0), note)
    assert o_rec.guards_intact(), (kernel, name, "guard records", note)
    return got


def pack(dev, W, kind):
    """mmego_pack_multi of one weight: kind 0 / 2 of W [Co][Ci][taps] -> 2 * numel floats (forward image, input-gradient image), kind 1 of
    W [Co][Ci] -> the fragment-major copy."""
    from mmego_amd import hip
    Wd = d_vec(dev, W)
    taps = W.shape[2] if W.dim() == 3 else 1
    o = Out(dev, 1, W.numel() * (1 if kind == 1 else 2), strided=False)
    p = hip.Pack(hip.ptr(Wd), hip.ptr(o.view), W.shape[0], W.shape[1], taps, kind)
    call("pack_multi", 1, (hip.Pack * 1)(p))
    assert o.guards_intact()
    return o.view.view(-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# shapes: the rules of the launchers restated, and the cases of this file held to them
# ---------------------------------------------------------------------------------------------------------------------------------
def front_inst(cin, nout, mix, K):
    """mmego_gcn_front's dispatch: (NCTW, NK) or None."""
    scalar = cin < 32
    phased = (not scalar) and mix
    nctw = K + 1 if phased else (nout // 32 + 3) // 4
    nk = 0 if scalar else cin // 32
    return (nctw, nk) if (nctw, nk) in {(1, 0), (3, 1), (3, 2), (1, 4), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2)} else None


def gather_round(NT, C):
    """Records one round of bn_gather / bn_gather2 / bwd_gather covers: 16 Q, Q = NT / CP, CP = the power of two >= max(C, 32)."""
    CP = 32
    while CP < C:
        CP <<= 1
    return 16 * (NT // CP)


def tconv_form(B, T, V, Cout):
    """tconv_launch: the four-step form (NG = 4) up to 512 tiles, else one step."""
    tiles = ((B * T * V + 63) // 64) * ((Cout + 63) // 64)
    return 4 if tiles <= 512 else 1


# gcn_front, in_mode 1: (F, V, T, cin, K, cout | nout, mix, rpr1, rpr2, sliced).  rpr1: the geometry of bn1's records (64-row tiles, per
# sequence T V, or a small number to reach a record count); rpr2: bn2's (4 V as the net, or small)
FRONT1 = [
    # mix = 1: K + 1 in {2, 3, 4} at cin 32 and 64 -> <2,1> <3,1> <4,1> <2,2> <3,2> <4,2>
    (37, 15, 1, 32, 1, 32, 1, 64, 60, False), (5, 7, 5, 32, 2, 64, 1, 35, 28, True), (3, 15, 3, 32, 3, 32, 1, 45, 60, False),
    (4, 15, 2, 64, 1, 64, 1, 30, 60, True), (37, 7, 37, 64, 2, 32, 1, 64, 28, False), (2, 1, 1, 64, 3, 128, 1, 64, 4, True),
    (1, 15, 1, 32, 2, 128, 1, 64, 60, False), (1, 1, 1, 64, 2, 64, 1, 1, 1, False),
    # record counts 1, 16 Q, 16 Q + 1 (the second gather round) and nrec1 != nrec2
    (512, 1, 1, 32, 1, 32, 1, 2, 4, False), (513, 1, 1, 32, 2, 32, 1, 2, 4, False),          # cin 32: Q = 16: 256 and 257 records
    (256, 1, 1, 64, 1, 32, 1, 2, 4, False), (257, 1, 1, 64, 2, 32, 1, 2, 4, True),           # cin 64: Q = 8: 128 and 129
    (37, 7, 1, 64, 1, 32, 1, 64, 2, False),                                                    # bn2 takes the second round alone (130 / 5)
    # mix = 0 (the closing conv, transposed store): <1,2> <1,4> <3,2> <2,1> <3,1> <2,2> <4,1> <4,2>
    (4, 15, 2, 64, 0, 128, 0, 30, 60, False), (37, 15, 37, 128, 0, 64, 0, 64, 60, True), (5, 7, 1, 64, 0, 384, 0, 7, 28, False),
    (3, 15, 3, 32, 0, 160, 0, 45, 60, True), (2, 7, 1, 32, 0, 320, 0, 7, 28, False), (1, 15, 1, 64, 0, 192, 0, 15, 60, False),
    (5, 1, 5, 32, 0, 416, 0, 5, 4, False), (2, 15, 2, 64, 0, 448, 0, 30, 60, True), (6, 15, 3, 64, 0, 64, 0, 45, 60, False),
    (256, 1, 2, 128, 0, 64, 0, 4, 4, False), (37, 7, 37, 128, 0, 128, 0, 4, 28, False),      # cin 128: Q = 4: 64 and 65 records
    (1, 7, 1, 128, 0, 64, 0, 64, 28, False),
]
# gcn_front, in_mode 0: (F, V, cin, K, cout, mix, nout, T)
FRONT0 = [(37, 15, 3, 2, 32, 1, 96, 1), (1, 15, 3, 2, 32, 1, 96, 1), (5, 7, 4, 1, 64, 1, 128, 1), (2, 1, 3, 1, 16, 1, 32, 1),
          (3, 15, 4, 3, 32, 1, 128, 1), (4, 7, 8, 0, 0, 0, 64, 2), (1024, 1, 5, 2, 32, 1, 96, 1)]
front1_id = lambda c: "F%d-V%d-T%d-cin%d-K%d-%d-mix%d-rpr%d.%d-%s" % (c[:9] + ("sliced" if c[9] else "dense",))
front0_id = lambda c: "F%d-V%d-cin%d-K%d-cout%d-mix%d-nout%d-T%d" % c

# the tile kernel: (B, T, V, Cin, Cout, sliced)
TILE = [(1, 9, 15, 32, 32, False), (3, 9, 15, 32, 32, True), (1, 9, 15, 64, 64, True), (3, 9, 15, 64, 64, False), (1, 9, 15, 128, 128, False),
        (3, 9, 15, 128, 128, True), (3, 9, 15, 36, 72, False), (1, 9, 15, 72, 36, True), (56, 10, 15, 32, 256, False), (56, 10, 15, 256, 32, False)]
# the sequence kernel: (B, T, V, Cin, Cout, sliced)
SEQ = [(1, 8, 15, 32, 32, False), (3, 8, 15, 64, 64, True), (3, 5, 15, 128, 128, False), (1, 5, 15, 64, 64, True), (3, 1, 15, 32, 32, True),
       (1, 1, 15, 128, 128, False), (3, 127, 1, 32, 32, False), (1, 127, 1, 64, 64, True), (1, 127, 1, 128, 128, True), (3, 8, 15, 32, 64, False),
       (1, 5, 15, 128, 64, True)]
tc_id = lambda c: "B%d-T%d-V%d-%dx%d-%s" % (c[:5] + ("sliced" if c[5] else "dense",))

BNB_ROWS, BNB_C = [1, 63, 64, 65, 135, 8193], [4, 32, 64, 128]
GDA_G, GDA_V, GDA_K, GDA_C = [1, 2, 3, 37], [15, 7, 1], [1, 2, 3], [16, 32, 64, 128]
BNP_ROWS, BNP_C = [1, 127, 128, 129, 1024], [1, 45, 48, 64]


def test_shape_rules(dev):
    """The launchers' rules restated in Python against the library where it exports them, and the cases above are the cases they claim."""
    from mmego_amd import hip
    lib = hip.lib()
    for F in (1, 2, 3, 4, 5, 37, 256, 513, 1024):
        assert lib.mmego_gcn_front_nrec(F) == (F + 3) // 4
    # every instantiation of the dispatch table is reached by a named case, the phased ones with K = 1, 2 and 3
    got = {front_inst(c[3], (c[4] + 1) * c[5] if c[6] else c[5], c[6], c[4]) for c in FRONT1} | {front_inst(c[2], c[6], c[5], c[3]) for c in FRONT0}
    assert got == {(1, 0), (3, 1), (3, 2), (1, 4), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2)}
    assert {(c[3], c[4]) for c in FRONT1 if c[6]} == {(ci, k) for ci in (32, 64) for k in (1, 2, 3)}
    assert {(c[3], c[5]) for c in FRONT1 if not c[6]} >= {(128, 64), (64, 128), (64, 384)}
    assert {c[0] for c in FRONT1 + FRONT0} >= {1, 2, 3, 4, 5, 37} and {c[1] for c in FRONT1} == {15, 7, 1}
    assert any(c[2] * c[6] == 512 for c in FRONT0) and (37, 15, 3, 2, 32, 1, 96, 1) in FRONT0
    # record counts: 1, 16 Q and 16 Q + 1 per channel count, unequal counts, the ragged last record
    counts = {(c[3], -(-c[0] * c[1] // c[7])) for c in FRONT1} | {(c[3], -(-c[0] * c[1] // c[8])) for c in FRONT1}
    for cin in (32, 64, 128):
        rnd = gather_round(512, cin)
        assert rnd == {32: 256, 64: 128, 128: 64}[cin]
        assert {(cin, 1), (cin, rnd), (cin, rnd + 1)} <= counts, cin
    assert any(-(-c[0] * c[1] // c[7]) != -(-c[0] * c[1] // c[8]) for c in FRONT1)
    assert any((c[0] * c[1]) % c[7] for c in FRONT1) and any((c[0] * c[1]) % c[8] for c in FRONT1)
    assert any(c[7] == 64 for c in FRONT1) and any(c[7] == c[2] * c[1] and c[2] > 1 for c in FRONT1) and any(c[8] == 4 * c[1] for c in FRONT1)
    # temporal convolution: which kernel takes which shape
    for B, T, V, Cin, Cout, _ in TILE:
        assert not lib.mmego_tconv_seq_ok(T, V, Cin, Cout) and T * V >= 128, (T, V)
        assert (B * T * V) % 64 != 0
    assert {tconv_form(*c[:3], c[4]) for c in TILE} == {4, 1} and tconv_form(56, 10, 15, 256) == 1 and 56 * 10 * 15 == 8400
    assert {tconv_form(*c[:3], c[3]) for c in TILE} == {4, 1}          # (the input-gradient call's column count is the convolution's Cin)
    assert {(c[3], c[4]) for c in TILE} >= {(32, 32), (64, 64), (128, 128), (36, 72), (72, 36)} and {c[0] for c in TILE if c[1] == 9} == {1, 3}
    for B, T, V, Cin, Cout, _ in SEQ:
        assert lib.mmego_tconv_seq_ok(T, V, Cin, Cout) and lib.mmego_tconv_seq_ok(T, V, Cout, Cin), (T, V, Cin, Cout)
    assert {(c[1], c[2]) for c in SEQ} == {(8, 15), (5, 15), (1, 15), (127, 1)} and {c[3] for c in SEQ} == {32, 64, 128} and {c[0] for c in SEQ} == {1, 3}
    # the boundary: the kernel's zero row is row 127 of its LDS tile, so 127 rows per sequence is the most it takes
    assert lib.mmego_tconv_seq_ok(127, 1, 32, 32) == 1 and lib.mmego_tconv_seq_ok(128, 1, 32, 32) == 0 and lib.mmego_tconv_seq_ok(8, 16, 64, 64) == 0
    assert lib.mmego_tconv_seq_ok(8, 15, 48, 64) == 0 and lib.mmego_tconv_seq_ok(8, 15, 64, 48) == 0 and lib.mmego_tconv_seq_ok(8, 15, 64, 288) == 0
    # gcn_bn_bwd: 8193 rows -> 129 records > 128 workgroups of the apply kernel (rows per workgroup 65, not 64), a second gather round at
    # C = 128 (CT = 256: 64 records per round)
    assert -(-8193 // 64) == 129 and gather_round(1024, 256) == 64 and gather_round(1024, 8) == 512
    assert -(-8193 // 128) == 65 and -(-8193 // 65) == 127
    # graph_dA_fused: 2 frames per workgroup; rounds of 128 / 64 / 32 records at C <= 32 / 64 / 128
    for G in GDA_G:
        assert lib.mmego_graph_dA_fused_nblk(G) == (G + 1) // 2
    assert [gather_round(256, C) for C in GDA_C] == [128, 128, 64, 32]


# ---------------------------------------------------------------------------------------------------------------------------------
# gcn_front
# ---------------------------------------------------------------------------------------------------------------------------------
def run_front1(dev, c, state=True, running=True, xact=True, bias=True):
    """gcn_front with in_mode 1 at case c -> dict of the outputs' CPU copies (after every check that the given outputs allow)."""
    from mmego_amd import hip
    F, V, T, cin, K, cw, mix, rpr1, rpr2, sliced = c
    cout = cw if mix else 0
    nout = (K + 1) * cw if mix else cw
    rows = F * V
    g = gen_for(21, *c)
    X1, X2 = randn(g, rows, cin, scale=1.1, shift=0.2), randn(g, rows, cin, scale=0.7, shift=-0.1)
    W, b = randn(g, nout, cin, scale=0.4), randn(g, nout, scale=0.3)
    bn1 = Bn(dev, g, cin, R.make_records(X1, rpr1), rpr1, state, running)
    bn2 = Bn(dev, g, cin, R.make_records(X2, rpr2), rpr2, state, running)
    A, imp = randn(g, max(K, 1), V, V, scale=0.4), torch.rand(max(K, 1), V, V, generator=g) + 0.5
    (dX1, ld1), (dX2, ld2) = d_mat(dev, X1, sliced), d_mat(dev, X2, True)            # X2: always a column slice, as res_z is in the net
    keep = [pack(dev, W, 1), d_vec(dev, b), d_vec(dev, A), d_vec(dev, imp)]
    nrf = (F + 3) // 4
    o_x = Out(dev, rows, cin, strided=False)
    d = hip.GcnFront()
    d.X1, d.ld1, d.X2, d.ld2, d.in_mode, d.bn1, d.bn2 = hip.ptr(dX1), ld1, hip.ptr(dX2), ld2, 1, bn1.ref, bn2.ref
    d.xact = hip.ptr(o_x.view) if xact else None
    d.W, d.bias, d.cin, d.nout, d.F, d.V = hip.ptr(keep[0]), hip.ptr(keep[1]) if bias else None, cin, nout, F, V
    if mix:
        o_z, o_y = Out(dev, rows, nout, sliced), Out(dev, rows, cout, strided=False)
        o_ry, o_rr = Out(dev, nrf, 2 * cout, strided=False, guard=2), Out(dev, nrf, 2 * cout, strided=False, guard=2)
        d.mix, d.K, d.cout, d.A, d.importance = 1, K, cout, hip.ptr(keep[2]), hip.ptr(keep[3])
        d.Z, d.ldz, d.Y, d.recY, d.recR = hip.ptr(o_z.view), o_z.ld, hip.ptr(o_y.view), hip.ptr(o_ry.view), hip.ptr(o_rr.view)
    else:
        o_t = Out(dev, (F // T) * nout, T * V, strided=False)
        d.mix, d.outT, d.T = 0, hip.ptr(o_t.view), T
    call("gcn_front", d)
    k, note = "gcn_front", front1_id(c) + ("" if state else " state=NULL") + ("" if running else " running=NULL") + ("" if xact else " xact=NULL")
    st1 = bn1.check(k, R.stats_from_records(bn1.rec, rows, rpr1, bn1.gamma, bn1.beta, bn1.rm0, bn1.rv0), note + " bn1")
    st2 = bn2.check(k, R.stats_from_records(bn2.rec, rows, rpr2, bn2.gamma, bn2.beta, bn2.rm0, bn2.rv0), note + " bn2")
    out = {"st1": st1, "st2": st2, "xact": o_x.cpu()}
    if mix:
        out.update(Z=o_z.cpu(), Y=o_y.cpu(), recY=o_ry.cpu(), recR=o_rr.cpu())
        assert o_z.guards_intact() and o_y.guards_intact() and o_ry.guards_intact() and o_rr.guards_intact(), note
    else:
        out.update(outT=o_t.cpu())
        assert o_t.guards_intact(), note
    assert o_x.guards_intact() if xact else o_x.untouched(), note
    if not state:
        return out
    x, xmag, cx = R.pair_act(X1, st1, X2, st2)
    if xact:
        check(k, "xact", out["xact"], x, cx * U32 * xmag, note)
    z, zb = R.product(x, xmag, cx, W, b if bias else None)
    if mix:
        check(k, "Z", out["Z"], z, zb, note)
        y, yb = R.einsum_mix(z, zb, A, imp, F, V, K, cout)
        check(k, "Y", out["Y"], y, yb, note)
        grp = R.groups(rows, 4 * V)
        check_records(k, "recY", o_ry, nrf, cout, *R.records_of(out["Y"], y, yb, grp), note)
        check_records(k, "recR", o_rr, nrf, cout, *R.records_of(out["Z"][:, K * cout:], z[:, K * cout:], zb[:, K * cout:], grp), note)
    else:
        tr = lambda t: t.reshape(F // T, T * V, nout).transpose(1, 2).reshape((F // T) * nout, T * V)
        check(k, "outT", out["outT"], tr(z), tr(zb), note)
    return out


@pytest.mark.parametrize("c", FRONT1, ids=front1_id)
def test_gcn_front_pair_input(dev, c):
    """in_mode 1: both BatchNorms' state and running statistics from their records (either geometry, ragged last record, one or two
    gather rounds), xact = max(bn1(X1) + bn2(X2), 0), the stacked product, and with mix = 1 the einsum and the records of Y and of the
    residual columns -- or with mix = 0 the transposed store."""
    run_front1(dev, c)


@pytest.mark.parametrize("c", [FRONT1[1], FRONT1[3], FRONT1[14]], ids=front1_id)
def test_gcn_front_optional_outputs(dev, c):
    """state, the running statistics, xact and the bias are optional: leaving any of them out changes no bit of what is still written
    (xact = NULL: not written; bias = NULL: the product against float64 without a bias)."""
    full = run_front1(dev, c)
    for kw in ({"state": False}, {"running": False}, {"xact": False}, {"state": False, "running": False, "xact": False}):
        got = run_front1(dev, c, **kw)
        for name in ("Z", "Y", "recY", "recR", "outT") + (("xact",) if kw.get("xact", True) else ()) + (("st1", "st2") if kw.get("state", True) else ()):
            if name in full:
                assert torch.equal(full[name], got[name]), (front1_id(c), kw, name)
    run_front1(dev, c, bias=False)


@pytest.mark.parametrize("c", FRONT0, ids=front0_id)
def test_gcn_front_data_bn(dev, c):
    """in_mode 0 (the scalar path, cin < 32): data_bn's statistics taken by the kernel over the F frames (state and running statistics
    against float64 of the frame tensor), xact = data_bn(X1) (no ReLU), the fp32 fma-chain product from the LDS copy of W, the einsum
    and both records; the largest weight the LDS copy holds (nout * cin = 512) included."""
    from mmego_amd import hip
    F, V, cin, K, cout, mix, nout, T = c
    rows, C = F * V, V * cin
    g = gen_for(22, *c)
    X = randn(g, F, C, scale=1.2, shift=0.3)
    W, b = randn(g, nout, cin, scale=0.4), randn(g, nout, scale=0.3)
    bn = Bn(dev, g, C, None, 0)
    A, imp = randn(g, max(K, 1), V, V, scale=0.4), torch.rand(max(K, 1), V, V, generator=g) + 0.5
    keep = [d_vec(dev, X), d_vec(dev, W), d_vec(dev, b), d_vec(dev, A), d_vec(dev, imp)]
    nrf = (F + 3) // 4
    o_x = Out(dev, rows, cin, strided=False)
    d = hip.GcnFront()
    d.X1, d.ld1, d.in_mode, d.bn1, d.xact = hip.ptr(keep[0]), C, 0, bn.ref, hip.ptr(o_x.view)
    d.W, d.bias, d.cin, d.nout, d.F, d.V = hip.ptr(keep[1]), hip.ptr(keep[2]), cin, nout, F, V
    if mix:
        o_z, o_y = Out(dev, rows, nout, True), Out(dev, rows, cout, strided=False)
        o_ry, o_rr = Out(dev, nrf, 2 * cout, strided=False, guard=2), Out(dev, nrf, 2 * cout, strided=False, guard=2)
        d.mix, d.K, d.cout, d.A, d.importance = 1, K, cout, hip.ptr(keep[3]), hip.ptr(keep[4])
        d.Z, d.ldz, d.Y, d.recY, d.recR = hip.ptr(o_z.view), o_z.ld, hip.ptr(o_y.view), hip.ptr(o_ry.view), hip.ptr(o_rr.view)
    else:
        o_t = Out(dev, (F // T) * nout, T * V, strided=False)
        d.mix, d.outT, d.T = 0, hip.ptr(o_t.view), T
    call("gcn_front", d)
    k, note = "gcn_front/data_bn", front0_id(c)
    st = bn.check(k, R.stats_direct(X, bn.gamma, bn.beta, bn.rm0, bn.rv0, -(-F // 8)), note)
    _, val, mag, _, _ = R.bn_parts(X, st)
    x, xmag = val.reshape(rows, cin), mag.reshape(rows, cin)
    check(k, "xact", o_x.cpu(), x, CACT * U32 * xmag, note)
    assert o_x.guards_intact(), note
    z, zb = R.product(x, xmag, CACT, W, b)
    if mix:
        check(k, "Z", o_z.cpu(), z, zb, note)
        y, yb = R.einsum_mix(z, zb, A, imp, F, V, K, cout)
        check(k, "Y", o_y.cpu(), y, yb, note)
        assert o_z.guards_intact() and o_y.guards_intact(), note
        grp = R.groups(rows, 4 * V)
        check_records(k, "recY", o_ry, nrf, cout, *R.records_of(o_y.cpu(), y, yb, grp), note)
        check_records(k, "recR", o_rr, nrf, cout, *R.records_of(o_z.cpu()[:, K * cout:], z[:, K * cout:], zb[:, K * cout:], grp), note)
    else:
        tr = lambda t: t.reshape(F // T, T * V, nout).transpose(1, 2).reshape((F // T) * nout, T * V)
        check(k, "outT", o_t.cpu(), tr(z), tr(zb), note)
        assert o_t.guards_intact(), note


# ---------------------------------------------------------------------------------------------------------------------------------
# temporal convolution: tconv_train / tconv_bwd_stats (64-row tiles) and tconv_seq_train / tconv_seq_bwd (one sequence per workgroup)
# ---------------------------------------------------------------------------------------------------------------------------------
def run_tconv_fwd(dev, seq, c, rpr_in, seed=31):
    """The training forward at case c through the sequence kernel (seq) or the tile kernel.  The BatchNorm in front comes as records of
    rpr_in rows each.  -> outputs, references and bounds."""
    B, T, V, Cin, Cout, sliced = c
    rows = B * T * V
    g = gen_for(seed, *c)
    X = randn(g, rows, Cin, scale=1.1, shift=0.2)
    W, b = randn(g, Cout, Cin, 9, scale=0.25), randn(g, Cout, scale=0.3)
    bn = Bn(dev, g, Cin, R.make_records(X, rpr_in), rpr_in)
    dX, ldx = d_mat(dev, X, sliced)
    wp, bd = pack(dev, W, 2 if seq else 0), d_vec(dev, b)
    rpr_out = T * V if seq else 64
    nro = -(-rows // rpr_out)
    o_y, o_a, o_r = Out(dev, rows, Cout, sliced), Out(dev, rows, Cin, strided=False), Out(dev, nro, 2 * Cout, strided=False, guard=2)
    k = "tconv_seq_train" if seq else "tconv_train"
    call(k, dX, ldx, bn.ref, wp[:W.numel()], bd, o_y.view, o_y.ld, o_a.view, o_r.view, B, T, V, Cin, Cout, 9)
    note = tc_id(c) + " rpr_in %d" % rpr_in
    stats = R.stats_from_records(bn.rec, rows, rpr_in, bn.gamma, bn.beta, bn.rm0, bn.rv0)
    st = bn.check(k, stats, note)
    _, val, mag, da, _ = R.bn_parts(X, st)
    check(k, "act", o_a.cpu(), val.clamp_min(0.0), U32 * (da + mag), note)
    y, yb = R.tconv(val.clamp_min(0.0), mag, CACT, W, b, B, T, V)
    check(k, "Y", o_y.cpu(), y, yb, note)
    assert o_y.guards_intact() and o_a.guards_intact(), note
    grp = R.groups(rows, rpr_out)
    rr, rb = R.records_of(o_y.cpu(), y, yb, grp)
    got = check_records(k, "out_rec", o_r, nro, Cout, rr, rb, note)
    return {"Y": o_y.cpu(), "y": (y, yb), "state": st, "stats": stats, "rec": got, "recref": (rr, rb), "grp": grp}


def run_tconv_bwd(dev, seq, c, seed=32):
    """The input-gradient call at case c (the convolution is Cin -> Cout: the kernel multiplies dY [rows][Cout] with the gradient image)
    with the (sum g, sum g xhat) records of the BatchNorm + ReLU in front of the convolution's input."""
    B, T, V, Cin, Cout, sliced = c
    rows = B * T * V
    g = gen_for(seed, *c)
    dY, ym, st = randn(g, rows, Cout), randn(g, rows, Cin, scale=1.1, shift=0.2), rand_state(g, Cin)
    W = randn(g, Cout, Cin, 9, scale=0.25)
    (ddY, lddy), (dym, ldym) = d_mat(dev, dY, sliced), d_mat(dev, ym, sliced)
    wp, std = pack(dev, W, 2 if seq else 0), d_vec(dev, st)
    rpr = T * V if seq else 64
    nr = -(-rows // rpr)
    o_d, o_r = Out(dev, rows, Cin, sliced), Out(dev, nr, 2 * Cin, strided=False, guard=2)
    k = "tconv_seq_bwd" if seq else "tconv_bwd_stats"
    call(k, ddY, lddy, wp[W.numel():], o_d.view, o_d.ld, dym, ldym, std, o_r.view, B, T, V, Cout, Cin, 9)
    note = tc_id(c)
    da, dab = R.tconv_input_grad(dY, W, B, T, V)
    check(k, "dAct", o_d.cpu(), da, dab, note)
    assert o_d.guards_intact(), note
    grp = R.groups(rows, rpr)
    rr, rb = R.g_records(o_d.cpu(), da, dab, ym, st, grp)
    got = check_records(k, "bw_rec", o_r, nr, Cin, rr, rb, note, summed=True)
    return {"dAct": o_d.cpu(), "da": (da, dab), "rec": got, "recref": (rr, rb)}


@pytest.mark.parametrize("c", TILE, ids=tc_id)
def test_tconv_train_tile(dev, c):
    """tconv_kernel<4, true, true> and, past 512 tiles, <1, true, true>: state and running statistics from gcn_front's records (4 V rows
    each), the activated rows, the convolution (ragged last 64-row tile, ragged channel chunk, Cout past a 64-column tile) and the
    (mean, M2) records of the output per 64-row tile."""
    run_tconv_fwd(dev, False, c, 4 * c[2])


@pytest.mark.parametrize("c", TILE, ids=tc_id)
def test_tconv_bwd_stats_tile(dev, c):
    """The tile kernel's input-gradient call and its bw_rec epilogue, per 64-row record and summed."""
    run_tconv_bwd(dev, False, c)


@pytest.mark.parametrize("c", SEQ, ids=tc_id)
def test_tconv_seq_train(dev, c):
    """tconv_seq_kernel<1 | 2 | 4, true>: as above with one record per sequence; T V = 127 fills the LDS tile up to its zero row."""
    run_tconv_fwd(dev, True, c, 4 * c[2])


@pytest.mark.parametrize("c", SEQ, ids=tc_id)
def test_tconv_seq_bwd(dev, c):
    """tconv_seq_kernel<1 | 2 | 4, false> and its bw_rec epilogue, per sequence and summed."""
    run_tconv_bwd(dev, True, c)


def combined(rec, bound, grp):
    """(mean, M2) records [n][C][2] and their bounds -> the statistics of all rows together and the bounds they imply."""
    n = torch.tensor([q[1] for q in grp], dtype=torch.float64).view(-1, 1)
    N = n.sum()
    r = rec.double()
    m = (n * r[:, :, 0]).sum(0) / N
    M2 = r[:, :, 1].sum(0) + (n * (r[:, :, 0] - m) ** 2).sum(0)
    bm = (n * bound[:, :, 0]).sum(0) / N
    bM2 = bound[:, :, 1].sum(0) + (2 * n * ((r[:, :, 0] - m).abs() + MARGIN * (bound[:, :, 0] + bm)) * (bound[:, :, 0] + bm)).sum(0)
    return m, bm, M2, bM2


@pytest.mark.parametrize("c", [(3, 8, 15, 32, 32, False), (3, 5, 15, 64, 64, True)], ids=tc_id)
def test_tconv_forms_agree(dev, c):
    """A shape both kernels take (the entry points of the tile kernel do not ask mmego_tconv_seq_ok): outputs and finalized state agree
    within the sum of their bounds, and the records of one form, taken together, equal the other's within bound."""
    a, b = run_tconv_fwd(dev, True, c, 4 * c[2]), run_tconv_fwd(dev, False, c, 4 * c[2])
    note = tc_id(c)
    check("tconv forms", "Y", a["Y"], b["Y"].double(), 2 * a["y"][1], note)
    check("tconv forms", "state", a["state"], b["state"].double(), 2 * a["stats"]["state"][1], note)
    ma, bma, Ma, bMa = combined(a["rec"], a["recref"][1], a["grp"])
    mb, bmb, Mb, bMb = combined(b["rec"], b["recref"][1], b["grp"])
    check("tconv forms", "out_rec mean", ma, mb, bma + bmb, note)
    check("tconv forms", "out_rec M2", Ma, Mb, bMa + bMb, note)
    a, b = run_tconv_bwd(dev, True, c), run_tconv_bwd(dev, False, c)
    check("tconv forms", "dAct", a["dAct"], b["dAct"].double(), 2 * a["da"][1], note)
    check("tconv forms", "bw_rec summed", a["rec"].double().sum(0), b["rec"].double().sum(0), a["recref"][1].sum(0) + b["recref"][1].sum(0), note)


# ---------------------------------------------------------------------------------------------------------------------------------
# gcn_bn_bwd_reduce / gcn_bn_bwd_apply
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", BNB_C)
@pytest.mark.parametrize("rows", BNB_ROWS)
def test_gcn_bn_bwd(dev, rows, C):
    """The closing pair's backward: the (sum g, sum g xhat) records per 64-row tile over the 2 C virtual channels, then d(gamma), d(beta)
    and dX of both BatchNorms from those records.  The mask is an input (the block's output); X2 is a column slice of a wider buffer."""
    g = gen_for(41, rows, C)
    sliced = bool((rows + C // 4) & 1)
    dY, X1, X2 = randn(g, rows, C), randn(g, rows, C, scale=1.1, shift=0.2), randn(g, rows, C, scale=0.8, shift=-0.3)
    mask = torch.relu(randn(g, rows, C))
    st1, st2 = rand_state(g, C), rand_state(g, C)
    (ddY, lddy), (dm, ldm), (dX1, ld1), (dX2, ld2) = d_mat(dev, dY, sliced), d_mat(dev, mask, sliced), d_mat(dev, X1, sliced), d_mat(dev, X2, True)
    s1, s2 = d_vec(dev, st1), d_vec(dev, st2)
    nrec = -(-rows // 64)
    o_r = Out(dev, nrec, 4 * C, strided=False, guard=2)
    pair = (ddY, lddy, dm, ldm, dX1, ld1, s1, dX2, ld2, s2, rows, C)
    call("gcn_bn_bwd_reduce", *pair, o_r.view)
    note, grp, mk = "%d x %d %s" % (rows, C, "sliced" if sliced else "dense"), R.groups(rows, 64), (mask > 0).double()
    zero = torch.zeros(rows, C, dtype=torch.float64)
    r1, b1 = R.g_records(dY, dY.double(), zero, X1, st1, grp, mk)
    r2, b2 = R.g_records(dY, dY.double(), zero, X2, st2, grp, mk)
    rec = check_records("gcn_bn_bwd_reduce", "rec", o_r, nrec, 2 * C, torch.cat((r1, r2), 1), torch.cat((b1, b2), 1), note, summed=True)
    o_g1, o_b1, o_g2, o_b2 = (Out(dev, 1, C, strided=False) for _ in range(4))
    o_x1, o_x2 = Out(dev, rows, C, sliced), Out(dev, rows, C, True)
    call("gcn_bn_bwd_apply", *pair, o_r.view, o_g1.view, o_b1.view, o_x1.view, o_x1.ld, o_g2.view, o_b2.view, o_x2.view, o_x2.ld)
    gm = dY.double() * mk
    k = "gcn_bn_bwd_apply"
    for nm, X, st, rr, og, ob, ox in (("1", X1, st1, rec[:, :C], o_g1, o_b1, o_x1), ("2", X2, st2, rec[:, C:], o_g2, o_b2, o_x2)):
        ref = R.bn_bwd(gm, X, st, rr, rows)
        check(k, "dgamma" + nm, og.cpu()[0], *ref["dgamma"], note)
        check(k, "dbeta" + nm, ob.cpu()[0], *ref["dbeta"], note)
        check(k, "dX" + nm, ox.cpu(), *ref["dX"], note)
        assert og.guards_intact() and ob.guards_intact() and ox.guards_intact(), (note, nm)
    assert o_r.guards_intact(), note


# ---------------------------------------------------------------------------------------------------------------------------------
# graph_dA_fused
# ---------------------------------------------------------------------------------------------------------------------------------
_POISON = {}


def poison_lds(dev):
    """Leave non-finite values in the LDS of every compute unit: tconv_seq_bwd on an all-NaN gradient stages 127 rows of NaN in 128 x
    132 floats of LDS per workgroup (more than graph_dA_fused ever uses), 1024 workgroups.  graph_dA_fused called right behind it sees NaN
    wherever it reads LDS it has not written."""
    if not _POISON:
        B, C = 1024, 128
        _POISON.update(dY=torch.full((B * 127, C), NAN, device=dev), W=torch.zeros(9 * C * 32, device=dev), st=torch.zeros(4 * 32, device=dev),
                       dA=torch.empty(B * 127, 32, device=dev), ym=torch.zeros(B * 127, 32, device=dev), rec=torch.empty(B, 32, 2, device=dev), B=B)
    p = _POISON
    call("tconv_seq_bwd", p["dY"], 128, p["W"], p["dA"], 32, p["ym"], 32, p["st"], p["rec"], p["B"], 127, 1, 128, 32, 9)


def run_graph_dA(dev, G, V, K, C, nrec, sliced, poison):
    g = gen_for(51, G, V, K, C, nrec)
    rows = G * V
    Z, dY0, ym, st = randn(g, rows, K * C, scale=0.9), randn(g, rows, C), randn(g, rows, C, scale=1.1, shift=0.2), rand_state(g, C)
    rec = randn(g, nrec, C, 2, scale=0.3 * rows / nrec)
    A, imp = randn(g, K, V, V, scale=0.4), torch.rand(K, V, V, generator=g) + 0.5
    dZ_, ldz = d_mat(dev, Z, sliced)
    ops = [d_vec(dev, dY0), d_vec(dev, ym), d_vec(dev, st), d_rec(dev, rec), d_vec(dev, A), d_vec(dev, imp)]
    nblk = (G + 1) // 2
    o_g, o_b = Out(dev, 1, C, strided=False), Out(dev, 1, C, strided=False)
    o_p, o_dz = Out(dev, nblk, K * V * V, strided=False, guard=2), Out(dev, rows, K * C, sliced)
    if poison:
        poison_lds(dev)
    call("graph_dA_fused", dZ_, ldz, ops[0], ops[1], ops[2], ops[3], nrec, o_g.view, o_b.view, G, V, K, C, o_p.view, ops[4], ops[5], o_dz.view, o_dz.ld)
    k, note = "graph_dA_fused", "G%d V%d K%d C%d nrec%d %s" % (G, V, K, C, nrec, "sliced" if sliced else "dense")
    mask = R.bn_parts(ym, st)[0]
    ref = R.bn_bwd(dY0.double() * mask, ym, st, rec, rows)
    check(k, "dgamma", o_g.cpu()[0], *ref["dgamma"], note)
    check(k, "dbeta", o_b.cpu()[0], *ref["dbeta"], note)
    gd = R.graph_dA(Z, ref["dX"][0], ref["dXmag"], A, imp, G, V, K, C)
    check(k, "dZ", o_dz.cpu(), *gd["dZ"], note)
    got = o_p.cpu().view(nblk, K, V, V)
    check(k, "partial", got, *gd["partial"], note)
    dA = torch.einsum("gvkc,gwc->kvw", Z.double().reshape(G, V, K, C), ref["dX"][0].reshape(G, V, C))        # the einsum's gradient, whole
    check(k, "partial summed", got.double().sum(0), dA, gd["partial"][1].sum(0), note)
    for o in (o_g, o_b, o_p, o_dz):
        assert o.guards_intact(), note


@pytest.mark.parametrize("K", GDA_K)
@pytest.mark.parametrize("V", GDA_V)
def test_graph_dA_fused(dev, V, K):
    """Every (G, C) of the table at this (V, K): d(gamma), d(beta) from the records, dZ, the dA partials per workgroup and summed against
    the float64 gradient of the einsum.  V < 15: behind a launch that left NaN in LDS -- the rows V .. 15 of both LDS tiles are the
    kernel's to zero (on the parent commit rows V .. 14 were not: NaN in dZ).  (V, K) = (15, 3) is past the entry point's K V V <= 512:
    refused, see test_other_refusals."""
    for G in GDA_G:
        for C in GDA_C:
            if K * V * V > 512 or V * K * C // 4 > 1024:  # (the entry point's limits: refused -- test_other_refusals)
                assert (V, K) == (15, 3)
                continue
            run_graph_dA(dev, G, V, K, C, 1 + (G * C + K) % 5, bool((G + C // 16 + K) & 1), V < 15)


@pytest.mark.parametrize("C", GDA_C)
def test_graph_dA_fused_record_counts(dev, C):
    """nrec = 1, 16 Q and 16 Q + 1 for the Q = 256 / CP of this channel count: the second round of bwd_gather."""
    rnd = gather_round(256, C)
    for nrec in (1, rnd, rnd + 1, 1024):
        run_graph_dA(dev, 3, 15, 2, C, nrec, False, False)


# ---------------------------------------------------------------------------------------------------------------------------------
# bn_param_grads / bn_input_grad
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", BNP_C)
@pytest.mark.parametrize("rows", BNP_ROWS)
def test_bn_param_and_input_grads(dev, rows, C):
    """d(gamma), d(beta) (fp64 accumulation of fp32 summands) and, from them, dX = a (dY - dbeta / rows - xhat dgamma / rows); operands
    dense and as column slices at an unaligned base (the entry points ask for no alignment)."""
    g = gen_for(61, rows, C)
    sliced = bool((rows + C) & 1)
    dY, X, st = randn(g, rows, C), randn(g, rows, C, scale=1.1, shift=0.2), rand_state(g, C)
    (ddY, lddy), (dX_, ldx) = d_mat(dev, dY, sliced, al=False), d_mat(dev, X, sliced, al=False)
    std = d_vec(dev, st)
    o_g, o_b = Out(dev, 1, C, strided=False), Out(dev, 1, C, strided=False)
    call("bn_param_grads", ddY, lddy, dX_, ldx, std, rows, C, o_g.view, o_b.view)
    note = "%d x %d %s" % (rows, C, "sliced" if sliced else "dense")
    xhat = R.bn_parts(X, st)[4]
    gd = dY.double()
    S1, S2 = gd.sum(0), (gd * xhat).sum(0)
    a1, a2 = gd.abs().sum(0), (gd * xhat).abs().sum(0)
    check("bn_param_grads", "dbeta", o_b.cpu()[0], S1, U32 * S1.abs() + rows * U64 * a1, note)
    check("bn_param_grads", "dgamma", o_g.cpu()[0], S2, U32 * S2.abs() + 3 * U32 * a2 + rows * U64 * a2, note)
    assert o_g.guards_intact() and o_b.guards_intact(), note
    o_x = Out(dev, rows, C, sliced, al=False)
    call("bn_input_grad", ddY, lddy, dX_, ldx, std, rows, C, o_g.view, o_b.view, o_x.view, o_x.ld)
    rec = torch.stack((o_b.cpu()[0], o_g.cpu()[0]), 1).view(1, C, 2)            # (the kernel's own sums are its inputs here)
    ref = R.bn_bwd(gd, X, st, rec, rows)
    check("bn_input_grad", "dX", o_x.cpu(), *ref["dX"], note)
    assert o_x.guards_intact() and o_g.guards_intact() and o_b.guards_intact(), note


# ---------------------------------------------------------------------------------------------------------------------------------
# slab_reduce, pack_multi
# ---------------------------------------------------------------------------------------------------------------------------------
def slab_entries(dev, g, specs):
    """specs: (kind, nsplit, M, N, taps, scm, asum, scale) -> (Slab descriptors, [(Out, reference, bound, name)], kept tensors)."""
    from mmego_amd import hip
    descs, outs, keep = [], [], []
    for i, (kind, nsplit, M, N, taps, scm, asum, scale) in enumerate(specs):
        ws = randn(g, nsplit * M * N + (nsplit * M if asum else 0))
        s = ws[:nsplit * M * N].view(nsplit, M * N).double()
        chain = -(-nsplit // 16) + 16
        ref, bound = s.sum(0), chain * U32 * s.abs().sum(0)
        sc = None
        if kind == 0:
            o = Out(dev, M, N, strided=False) if scm == N else Out(dev, M, scm, strided=False)
            view = o.view[:, :N]
            ref, bound = ref.view(M, N), bound.view(M, N)
        elif kind == 1:
            Co = M // taps
            o = Out(dev, Co, N * taps, strided=False)
            view = o.view
            ref, bound = (t.view(taps, Co, N).permute(1, 2, 0).reshape(Co, N * taps) for t in (ref, bound))
        else:
            o = Out(dev, 1, N, strided=False)
            view = o.view
            ref, bound = ref.view(1, N), bound.view(1, N)
            if scale:
                sc = randn(g, N)
                ref, bound = ref * sc.double(), (chain + 1) * U32 * s.abs().sum(0).view(1, N) * sc.abs().double()
        oa = None
        if asum:
            oa = Out(dev, 1, M, strided=False)
            sa = ws[nsplit * M * N:].view(nsplit, M).double()
            outs.append((oa, oa.view, sa.sum(0).view(1, M), chain * U32 * sa.abs().sum(0).view(1, M), "asum entry %d" % i))
        wsd = d_vec(dev, ws)
        scd = None if sc is None else d_vec(dev, sc)
        keep += [wsd, scd]
        descs.append(hip.Slab(hip.ptr(wsd), hip.ptr(o.view), hip.ptr(scd), hip.ptr(None if oa is None else oa.view), kind, nsplit, M, N, taps, scm))
        outs.append((o, view, ref, bound, "kind %d entry %d" % (kind, i)))
    return descs, outs, keep


def test_slab_reduce(dev):
    """All three kinds in one 24-entry table: nsplit 1 / 16 / 17 / 128 / 129 (the eight-deep unrolled loop and its tail), M N no multiple of
    16, scm > N (the columns between are not written), slab row sums (asum), the scaled column sums; 25 entries are refused."""
    from mmego_amd import hip
    g = gen_for(71)
    specs = []
    for i, ns in enumerate((1, 16, 17, 128, 129)):
        specs.append((0, ns, 5, 7, 1, 7 if i & 1 else 11, bool(i & 1), False))
        specs.append((1, ns, 9 * 4, 5, 9, 0, False, False))
        specs.append((2, ns, 1, 3 * 15 * 15 if i == 0 else 37, 1, 0, False, i != 1))
    specs += [(0, 129, 16, 16, 1, 16, True, False), (0, 3, 1, 1, 1, 1, True, False), (1, 2, 3, 33, 1, 0, False, False), (2, 240, 1, 675, 1, 0, False, True)]
    specs += [(0, 130 + i, 3, 5, 1, 9, True, False) for i in range(24 - len(specs))]
    assert len(specs) == 24
    descs, outs, keep = slab_entries(dev, g, specs)
    call("slab_reduce", 24, (hip.Slab * 24)(*descs))
    for o, view, ref, bound, name in outs:
        check("slab_reduce", name.split(" entry")[0], view.cpu(), ref, bound, name)
        b = o.buf.clone().view(o.rows + o.guard, o.ld)
        b[:o.rows][:, :view.shape[1]] = SENT
        assert bool((b == SENT).all()), name
    o25 = Out(dev, 1, 4, strided=False)
    refused("slab_reduce", 25, (hip.Slab * 25)(*(descs + [descs[0]])))
    refused("slab_reduce", 0, (hip.Slab * 1)(descs[0]))
    bad = hip.Slab(descs[1].ws, descs[1].out, None, None, 1, 2, 10, 5, 3, 0)                    # kind 1: M no multiple of taps
    refused("slab_reduce", 1, (hip.Slab * 1)(bad))
    bad = hip.Slab(descs[1].ws, descs[1].out, None, hip.ptr(o25.view), 1, 2, 9, 5, 9, 0)        # asum with another kind than 0
    refused("slab_reduce", 1, (hip.Slab * 1)(bad))
    assert o25.untouched()


@pytest.mark.parametrize("kind,Co,Ci,taps", [(1, 96, 32, 1), (1, 64, 128, 1), (1, 384, 64, 1), (2, 32, 32, 9), (2, 96, 64, 9), (0, 72, 36, 9)])
def test_pack_multi_is_a_permutation(dev, kind, Co, Ci, taps):
    """Every source element appears exactly once in the packed image (kinds 0 and 2: once in the forward image and once in the
    input-gradient image).  The images' layouts themselves are checked through the products above, whose references multiply with the
    unpacked weights."""
    n = Co * Ci * taps
    W = (torch.arange(n, dtype=torch.float32) + 1.0).view((Co, Ci, taps) if taps > 1 else (Co, Ci))
    wp = pack(dev, W, kind).cpu()
    want = torch.arange(n, dtype=torch.float32) + 1.0
    for img in ((wp,) if kind == 1 else (wp[:n], wp[n:])):
        assert torch.equal(img.sort().values, want), (kind, Co, Ci)
    if kind == 0:                                         # tap-major: [tap][co][ci], then [taps - 1 - tap][ci][co]
        assert torch.equal(wp[:n].view(taps, Co, Ci), W.permute(2, 0, 1)) and torch.equal(wp[n:].view(taps, Ci, Co), W.permute(2, 1, 0).flip(0))


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: the limits each entry point states (return code, no launch: the outputs keep their sentinel)
# ---------------------------------------------------------------------------------------------------------------------------------
def front_desc(dev, keep, **kw):
    """A valid in_mode 1 / mix 1 descriptor (cin 32, K 2, cout 32, F 4, V 15) with the given fields replaced."""
    from mmego_amd import hip
    F, V, cin, K, cout = kw.pop("F", 4), kw.pop("V", 15), kw.pop("cin", 32), kw.pop("K", 2), kw.pop("cout", 32)
    nout = kw.pop("nout", (K + 1) * cout)
    rows = F * V
    big = lambda n: torch.zeros(max(n, 1) + 8, device=dev)
    x1, x2, w, b, A = big(rows * 128), big(rows * 128), big(512 * 128), big(512), big(3 * V * V)
    rec = torch.zeros(rows + 4, 128, 2, device=dev)
    gam = torch.ones(128, device=dev)
    outs = [Out(dev, rows, 512, strided=False, guard=1), Out(dev, rows, 128, strided=False, guard=1), Out(dev, (F + 3) // 4, 256, strided=False, guard=1),
            Out(dev, (F + 3) // 4, 256, strided=False, guard=1), Out(dev, rows, 128, strided=False, guard=1)]
    keep += [x1, x2, w, b, A, rec, gam] + outs
    bn = hip.BnRef(rec=hip.ptr(rec), nrec=(rows + 63) // 64, rows_per_rec=64, gamma=hip.ptr(gam), beta=hip.ptr(gam), running_mean=None, running_var=None,
                   momentum=MOM, eps=EPS, state=None)
    d = hip.GcnFront()
    d.X1, d.ld1, d.X2, d.ld2, d.in_mode, d.bn1, d.bn2 = hip.ptr(x1), cin, hip.ptr(x2), cin, 1, bn, bn
    d.xact, d.W, d.bias, d.cin, d.nout = hip.ptr(outs[4].view), hip.ptr(w), hip.ptr(b), cin, nout
    d.mix, d.K, d.cout, d.A, d.importance = 1, K, cout, hip.ptr(A), hip.ptr(A)
    d.Z, d.ldz, d.Y, d.recY, d.recR = hip.ptr(outs[0].view), nout, hip.ptr(outs[1].view), hip.ptr(outs[2].view), hip.ptr(outs[3].view)
    d.outT, d.T, d.F, d.V = hip.ptr(outs[0].view), 1, F, V
    for k, v in kw.items():
        setattr(d, k, v)
    return d, outs


def test_gcn_front_refusals(dev):
    """What mmego_gcn_front refuses, with the shapes its kernels do not compute among them: the phased path (mix = 1, cin >= 32) needs cout
    a power of two >= 32 (16: no wave computes anything; 48: columns 32..47 missing), the scalar path nout * cin <= 512 and nout <= 128
    (its LDS copy of W is 512 floats, one element per thread) and cin <= 8 (its input tile has a row stride of 8 floats)."""
    keep = []
    d, outs = front_desc(dev, keep)
    call("gcn_front", d)                                   # (the base descriptor is valid)
    bad = [dict(cout=16), dict(cout=48), dict(cout=96), dict(K=1, cout=16), dict(cin=64, cout=48, K=1), dict(cin=64, cout=16, K=3),
           dict(V=16), dict(V=0), dict(F=0), dict(K=4), dict(K=0), dict(cin=48), dict(cin=160, K=1), dict(cin=128, K=1, cout=32),
           dict(nout=128), dict(ld1=34), dict(ld2=33), dict(in_mode=2), dict(Z=None), dict(recR=None), dict(A=None), dict(X2=None), dict(W=None),
           dict(ldz=64), dict(cout=256, K=1), dict(mix=0, nout=96, T=3), dict(mix=0, nout=96, T=0), dict(mix=0, nout=48), dict(mix=0, nout=96, outT=None),
           dict(mix=0, nout=96, cin=32)]                   # (<1,1> is not in the dispatch table)
    for kw in bad:
        d, outs = front_desc(dev, keep, **kw)
        refused("gcn_front", d)
        assert all(o.untouched() for o in outs), kw
    # in_mode 0: V cin <= 64, F <= 1024, gamma and beta; the LDS copy of W
    for kw in (dict(cin=5, V=12, K=3, cout=32), dict(cin=5, V=12, K=1, cout=64, F=2), dict(cin=3, V=15, K=2, cout=64), dict(cin=8, V=7, K=1, cout=48),
               dict(cin=5, V=15, K=2, cout=32), dict(cin=3, V=15, K=2, cout=32, F=1028), dict(cin=1, V=15, mix=0, nout=160, K=2, cout=32), dict(cin=16, V=4, K=1, cout=16), dict(cin=9, V=7, K=1, cout=16)):
        d, outs = front_desc(dev, keep, in_mode=0, **kw)
        refused("gcn_front", d)
        assert all(o.untouched() for o in outs), kw
    d, outs = front_desc(dev, keep, in_mode=0, cin=4, V=15, K=3, cout=32)           # nout * cin = 512 exactly: taken
    call("gcn_front", d)
    d, _ = front_desc(dev, keep, in_mode=0, cin=3, V=15, K=2, cout=32)
    d.bn1.gamma = None
    refused("gcn_front", d)
    d, _ = front_desc(dev, keep)
    d.bn2.nrec = 0
    refused("gcn_front", d)
    d, _ = front_desc(dev, keep)
    d.X1 = d.X1 + 4
    refused("gcn_front", d)
    torch.cuda.synchronize()


def test_other_refusals(dev):
    """The limits the other entry points of the fused step state."""
    from mmego_amd import hip
    z = torch.zeros(1 << 16, device=dev)
    o = Out(dev, 1, 1 << 16, strided=False, guard=0)
    bn = hip.BnRef(rec=hip.ptr(z), nrec=1, rows_per_rec=64, gamma=hip.ptr(z), beta=hip.ptr(z), running_mean=None, running_var=None, momentum=MOM, eps=EPS,
                   state=None)
    tc = lambda **kw: [kw.get(n, v) for n, v in (("X", z), ("ldx", 32), ("bn", bn), ("W", z), ("bias", None), ("Y", o.view), ("ldy", 32), ("act", None),
                                                 ("rec", o.view), ("B", 1), ("T", 8), ("V", 15), ("Cin", 32), ("Cout", 32), ("taps", 9))]
    for kw in (dict(T=128, V=1), dict(T=9), dict(T=8, V=16), dict(Cin=48, ldx=48), dict(Cout=48, ldy=48), dict(Cout=288, ldy=288), dict(taps=7), dict(ldx=28),
               dict(ldx=34), dict(ldy=30), dict(B=0), dict(rec=None), dict(W=None), dict(X=z[1:])):
        refused("tconv_seq_train", *tc(**kw))
    for kw in (dict(Cin=260, ldx=260), dict(Cin=30, ldx=32), dict(Cin=2, ldx=4), dict(ldx=34), dict(ldx=28), dict(ldy=30), dict(taps=8), dict(taps=0), dict(T=0),
               dict(rec=None), dict(X=z[1:])):
        refused("tconv_train", *tc(**kw))
    tb = lambda **kw: [kw.get(n, v) for n, v in (("dY", z), ("lddy", 32), ("W", z), ("dAct", o.view), ("ldda", 32), ("ym", z), ("ldym", 32), ("st", z),
                                                 ("rec", o.view), ("B", 1), ("T", 8), ("V", 15), ("Cin", 32), ("Cout", 32), ("taps", 9))]
    for kw in (dict(T=128, V=1), dict(Cin=96, lddy=96), dict(Cout=48, ldda=48, ldym=48), dict(ldda=34), dict(ldym=34), dict(lddy=28), dict(taps=3), dict(st=None),
               dict(ym=z[1:]), dict(dAct=o.view.view(-1)[1:])):
        refused("tconv_seq_bwd", *tb(**kw))
    for kw in (dict(Cin=30, lddy=32), dict(lddy=34), dict(lddy=28), dict(ldda=30), dict(ldym=30), dict(taps=4), dict(st=None), dict(rec=None), dict(dY=z[1:])):
        refused("tconv_bwd_stats", *tb(**kw))
    pr = lambda **kw: [kw.get(n, v) for n, v in (("dY", z), ("lddy", 32), ("mask", z), ("ldm", 32), ("X1", z), ("ld1", 32), ("st1", z), ("X2", z), ("ld2", 32),
                                                 ("st2", z), ("rows", 100), ("C", 32))]
    ap = [o.view, o.view, o.view, 32, o.view, o.view, o.view, 32]
    for kw in (dict(C=2), dict(C=30), dict(C=132), dict(rows=0), dict(st2=None), dict(mask=None)):
        refused("gcn_bn_bwd_reduce", *pr(**kw), o.view)
        refused("gcn_bn_bwd_apply", *pr(**kw), z, *ap)
    for kw in (dict(lddy=34), dict(ldm=34), dict(ld1=34), dict(ld2=34), dict(dY=z[1:]), dict(X2=z[1:]), dict(rows=64 * 1024 + 1)):
        refused("gcn_bn_bwd_apply", *pr(**kw), z, *ap)
    refused("gcn_bn_bwd_apply", *pr(), z, o.view, o.view, o.view, 34, o.view, o.view, o.view, 32)
    refused("gcn_bn_bwd_apply", *pr(), z, o.view, None, o.view, 32, o.view, o.view, o.view, 32)
    gd = lambda **kw: [kw.get(n, v) for n, v in (("Z", z), ("ldz", 64), ("dY0", z), ("ym", z), ("st", z), ("rec", z), ("nrec", 1), ("dg", o.view), ("db", o.view),
                                                 ("G", 2), ("V", 15), ("K", 2), ("C", 32), ("part", o.view), ("A", z), ("imp", z), ("dZ", o.view), ("lddz", 64))]
    for kw in (dict(V=16), dict(V=0), dict(K=4), dict(K=0), dict(C=24), dict(C=144), dict(C=0), dict(K=3, C=128, ldz=384, lddz=384), dict(K=3, ldz=96, lddz=96), dict(nrec=0), dict(nrec=1025), dict(ldz=60), dict(lddz=60),
               dict(ldz=66), dict(lddz=66), dict(G=0), dict(Z=z[1:]), dict(dZ=o.view.view(-1)[1:]), dict(ym=z[2:]), dict(rec=None), dict(A=None)):
        refused("graph_dA_fused", *gd(**kw))
    bp = [z, 8, z, 8, z, 10, 8]
    refused("bn_param_grads", z, 8, z, 8, z, 0, 8, o.view, o.view)
    refused("bn_param_grads", z, 8, z, 8, z, 10, 0, o.view, o.view)
    refused("bn_param_grads", z, 8, z, 8, None, 10, 8, o.view, o.view)
    for tail in ((z, z, o.view, 7), (z, z, None, 8), (None, z, o.view, 8)):
        refused("bn_input_grad", *bp, *tail)
    refused("bn_input_grad", z, 7, z, 8, z, 10, 8, z, z, o.view, 8)
    refused("bn_input_grad", z, 8, z, 7, z, 10, 8, z, z, o.view, 8)
    pk = lambda *a: (hip.Pack * 1)(hip.Pack(hip.ptr(z), hip.ptr(o.view), *a))
    for a in ((48, 32, 1, 1), (32, 48, 1, 1), (32, 32, 9, 1), (48, 32, 9, 2), (32, 32, 1, 3), (0, 32, 1, 0), (32, 32, 0, 0)):
        refused("pack_multi", 1, pk(*a))
    refused("pack_multi", 9, (hip.Pack * 9)(*[hip.Pack(hip.ptr(z), hip.ptr(o.view), 4, 4, 1, 0)] * 9))
    torch.cuda.synchronize()
    assert o.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------
# one block, forward and backward, every buffer handed from launch to launch on the device
# ---------------------------------------------------------------------------------------------------------------------------------
def block_by_references(x, P, A, imp, B, T, V, K, cout, masks, dout):
    """The block's gradients by the reference functions the kernels are held to, chained as the launches are chained, on float64
    operands (every "fp32" step of theirs is then exact) with the given ReLU masks."""
    F, rows = B * T, B * T * V
    one = lambda C: (torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64))
    zr = R.product(x, x.abs(), 0, P["Wc"], P["bc"])[0]
    ymix = R.einsum_mix(zr, torch.zeros_like(zr), A, imp, F, V, K, cout)[0]
    rec64 = lambda t, rpr: torch.stack([torch.stack((t[s:s + n].mean(0), ((t[s:s + n] - t[s:s + n].mean(0)) ** 2).sum(0)), 1) for s, n in R.groups(rows, rpr)])
    st0 = R.stats_from_records(rec64(ymix, 4 * V), rows, 4 * V, P["g0"], P["b0"], *one(cout))["state"][0]
    y0 = masks[0] * R.bn_parts(ymix, st0)[1]
    tz = R.tconv(y0, y0.abs(), 0, P["Wt"], P["bt"], B, T, V)[0]
    rz = zr[:, K * cout:]
    st3 = R.stats_from_records(rec64(tz, T * V), rows, T * V, P["g3"], P["b3"], *one(cout))["state"][0]
    str_ = R.stats_from_records(rec64(rz, 4 * V), rows, 4 * V, P["gr"], P["br"], *one(cout))["state"][0]
    g = dout * masks[1]
    zero, grp = torch.zeros_like(g), R.groups(rows, 64)
    r3 = R.g_records(g, g, zero, tz, st3, grp, torch.ones_like(g))[0]
    rr = R.g_records(g, g, zero, rz, str_, grp, torch.ones_like(g))[0]
    b3, br = R.bn_bwd(g, tz, st3, r3, rows), R.bn_bwd(g, rz, str_, rr, rows)
    dy0 = R.tconv_input_grad(b3["dX"][0], P["Wt"], B, T, V)[0]
    r0 = R.g_records(dy0, dy0, torch.zeros_like(dy0), ymix, st0, R.groups(rows, T * V), masks[0])[0]
    b0 = R.bn_bwd(dy0 * masks[0], ymix, st0, r0, rows)
    gd = R.graph_dA(zr[:, :K * cout], b0["dX"][0], b0["dXmag"], A, imp, F, V, K, cout)
    return {"dz": gd["dZ"][0], "drz": br["dX"][0], "dAimp": gd["partial"][0].sum(0), "dg0": b0["dgamma"][0], "db0": b0["dbeta"][0],
            "dg3": b3["dgamma"][0], "db3": b3["dbeta"][0], "dgr": br["dgamma"][0], "dbr": br["dbeta"][0], "dtz": b3["dX"][0], "dy0": dy0}


def test_block_chain(dev):
    """gcn_front -> tconv_seq_train -> the next gcn_front (which closes the block: out = relu(bn3(tz) + bnr(rz))), then gcn_bn_bwd_reduce /
    apply -> tconv_seq_bwd -> graph_dA_fused at B = 2, T = 5, V = 15 (10 frames: a ragged last 4-frame tile; 150 rows: a ragged 64-row
    record), cin = 32, K = 2, cout = 64, every buffer handed on on the device.

    Tolerance: STAGE-WISE.  Every launch's outputs are held to the float64 formula of that launch fed the device's own inputs of that
    launch, with the bounds of the single-kernel tests; the masks come from the device's own values by the sign identity.  What ties
    the stages to the block is the last part: the same reference functions, chained on float64 operands with those masks, reproduce
    float64 autograd of the block written with torch ops (gcn_train_ref.block_torch) to 1e-9 of the largest element."""
    from mmego_amd import hip
    B, T, V, cin, K, cout = 2, 5, 15, 32, 2, 64
    F, rows, nout = B * T, B * T * V, (K + 1) * cout
    g = gen_for(81)
    X1, X2 = randn(g, rows, cin, scale=1.1, shift=0.2), randn(g, rows, cin, scale=0.7, shift=-0.1)
    Wc, bc = randn(g, nout, cin, scale=0.4), randn(g, nout, scale=0.3)
    Wt, bt = randn(g, cout, cout, 9, scale=0.2), randn(g, cout, scale=0.3)
    A, imp = randn(g, K, V, V, scale=0.4), torch.rand(K, V, V, generator=g) + 0.5
    Wn = randn(g, 64, cout, scale=0.3)
    dout = randn(g, rows, cout)
    bnA = Bn(dev, g, cin, R.make_records(X1, T * V), T * V)
    bnB = Bn(dev, g, cin, R.make_records(X2, 4 * V), 4 * V)
    nrf = (F + 3) // 4
    keep = [d_vec(dev, t) for t in (X1, X2, bc, A, imp)] + [pack(dev, Wc, 1), pack(dev, Wt, 2), d_vec(dev, bt), pack(dev, Wn, 1)]
    o_x, o_zr, o_ym = Out(dev, rows, cin, strided=False), Out(dev, rows, nout, strided=False), Out(dev, rows, cout, strided=False)
    o_ry, o_rr = Out(dev, nrf, 2 * cout, strided=False, guard=2), Out(dev, nrf, 2 * cout, strided=False, guard=2)
    d = hip.GcnFront()
    d.X1, d.ld1, d.X2, d.ld2, d.in_mode, d.bn1, d.bn2, d.xact = hip.ptr(keep[0]), cin, hip.ptr(keep[1]), cin, 1, bnA.ref, bnB.ref, hip.ptr(o_x.view)
    d.W, d.bias, d.cin, d.nout, d.F, d.V = hip.ptr(keep[5]), hip.ptr(keep[2]), cin, nout, F, V
    d.mix, d.K, d.cout, d.A, d.importance = 1, K, cout, hip.ptr(keep[3]), hip.ptr(keep[4])
    d.Z, d.ldz, d.Y, d.recY, d.recR = hip.ptr(o_zr.view), nout, hip.ptr(o_ym.view), hip.ptr(o_ry.view), hip.ptr(o_rr.view)
    call("gcn_front", d)
    bn0 = Bn(dev, g, cout, None, 4 * V)
    bn0.ref.rec, bn0.ref.nrec = hip.ptr(o_ry.view), nrf
    o_tz, o_y0, o_r3 = Out(dev, rows, cout, strided=False), Out(dev, rows, cout, strided=False), Out(dev, B, 2 * cout, strided=False, guard=2)
    call("tconv_seq_train", o_ym.view, cout, bn0.ref, keep[6][:Wt.numel()], keep[7], o_tz.view, cout, o_y0.view, o_r3.view, B, T, V, cout, cout, 9)
    bn3, bnr = Bn(dev, g, cout, None, T * V), Bn(dev, g, cout, None, 4 * V)
    bn3.ref.rec, bn3.ref.nrec, bnr.ref.rec, bnr.ref.nrec = hip.ptr(o_r3.view), B, hip.ptr(o_rr.view), nrf
    o_out, o_kv = Out(dev, rows, cout, strided=False), Out(dev, B * 64, T * V, strided=False)
    d2 = hip.GcnFront()
    d2.X1, d2.ld1, d2.X2, d2.ld2, d2.in_mode, d2.bn1, d2.bn2 = hip.ptr(o_tz.view), cout, hip.ptr(o_zr.view[:, K * cout:]), nout, 1, bn3.ref, bnr.ref
    d2.xact, d2.W, d2.bias, d2.cin, d2.nout, d2.F, d2.V = hip.ptr(o_out.view), hip.ptr(keep[8]), None, cout, 64, F, V
    d2.mix, d2.outT, d2.T = 0, hip.ptr(o_kv.view), T
    call("gcn_front", d2)
    # backward
    ddout = d_vec(dev, dout).view(rows, cout)
    nrt = -(-rows // 64)
    o_br = Out(dev, nrt, 4 * cout, strided=False, guard=2)
    o_dzr = Out(dev, rows, nout, strided=False)
    o_dtz = Out(dev, rows, cout, strided=False)
    o_g3, o_b3, o_gr, o_brr, o_g0, o_b0 = (Out(dev, 1, cout, strided=False) for _ in range(6))
    pair = (ddout, cout, o_out.view, cout, o_tz.view, cout, bn3.o_state.view, o_zr.view[:, K * cout:], nout, bnr.o_state.view, rows, cout, o_br.view)
    call("gcn_bn_bwd_reduce", *pair)
    call("gcn_bn_bwd_apply", *pair, o_g3.view, o_b3.view, o_dtz.view, cout, o_gr.view, o_brr.view, o_dzr.view[:, K * cout:], nout)
    o_dy0, o_bw = Out(dev, rows, cout, strided=False), Out(dev, B, 2 * cout, strided=False, guard=2)
    call("tconv_seq_bwd", o_dtz.view, cout, keep[6][Wt.numel():], o_dy0.view, cout, o_ym.view, cout, bn0.o_state.view, o_bw.view, B, T, V, cout, cout, 9)
    nda = (F + 1) // 2
    o_pa = Out(dev, nda, K * V * V, strided=False, guard=2)
    call("graph_dA_fused", o_zr.view, nout, o_dy0.view, o_ym.view, bn0.o_state.view, o_bw.view, B, o_g0.view, o_b0.view, F, V, K, cout, o_pa.view,
         keep[3], keep[4], o_dzr.view, nout)
    torch.cuda.synchronize()
    k = "chain"
    # ---- forward, stage by stage
    stA = bnA.check(k, R.stats_from_records(bnA.rec, rows, T * V, bnA.gamma, bnA.beta, bnA.rm0, bnA.rv0), "front bn1")
    stB = bnB.check(k, R.stats_from_records(bnB.rec, rows, 4 * V, bnB.gamma, bnB.beta, bnB.rm0, bnB.rv0), "front bn2")
    x, xmag, cx = R.pair_act(X1, stA, X2, stB)
    check(k, "xact", o_x.cpu(), x, cx * U32 * xmag)
    z, zb = R.product(x, xmag, cx, Wc, bc)
    zr = o_zr.cpu()
    check(k, "Z", zr, z, zb)
    y, yb = R.einsum_mix(z, zb, A, imp, F, V, K, cout)
    ym = o_ym.cpu()
    check(k, "Y", ym, y, yb)
    grp4 = R.groups(rows, 4 * V)
    recY = check_records(k, "recY", o_ry, nrf, cout, *R.records_of(ym, y, yb, grp4), "")
    recR = check_records(k, "recR", o_rr, nrf, cout, *R.records_of(zr[:, K * cout:], z[:, K * cout:], zb[:, K * cout:], grp4), "")
    st0 = bn0.check(k, R.stats_from_records(recY, rows, 4 * V, bn0.gamma, bn0.beta, bn0.rm0, bn0.rv0), "bn0")
    m0, val, mag, da, _ = R.bn_parts(ym, st0)
    check(k, "y0", o_y0.cpu(), val.clamp_min(0.0), U32 * (da + mag))
    tzr, tzb = R.tconv(val.clamp_min(0.0), mag, CACT, Wt, bt, B, T, V)
    tz = o_tz.cpu()
    check(k, "tz", tz, tzr, tzb)
    rec3 = check_records(k, "rec3", o_r3, B, cout, *R.records_of(tz, tzr, tzb, R.groups(rows, T * V)), "")
    st3 = bn3.check(k, R.stats_from_records(rec3, rows, T * V, bn3.gamma, bn3.beta, bn3.rm0, bn3.rv0), "bn3")
    str_ = bnr.check(k, R.stats_from_records(recR, rows, 4 * V, bnr.gamma, bnr.beta, bnr.rm0, bnr.rv0), "bnr")
    rz = zr[:, K * cout:].contiguous()
    outr, outm, co = R.pair_act(tz, st3, rz, str_)
    out = o_out.cpu()
    check(k, "out", out, outr, co * U32 * outm)
    kvr, kvb = R.product(outr, outm, co, Wn, None)
    tr = lambda t: t.reshape(B, T * V, 64).transpose(1, 2).reshape(B * 64, T * V)
    check(k, "kv", o_kv.cpu(), tr(kvr), tr(kvb))
    # ---- backward, stage by stage, each fed what the chain handed it
    mout = (out > 0).double()
    zero = torch.zeros(rows, cout, dtype=torch.float64)
    r3, b3_ = R.g_records(dout, dout.double(), zero, tz, st3, R.groups(rows, 64), mout)
    rr, br_ = R.g_records(dout, dout.double(), zero, rz, str_, R.groups(rows, 64), mout)
    brec = check_records(k, "brec", o_br, nrt, 2 * cout, torch.cat((r3, rr), 1), torch.cat((b3_, br_), 1), "", summed=True)
    gm = dout.double() * mout
    ref3, refr = R.bn_bwd(gm, tz, st3, brec[:, :cout], rows), R.bn_bwd(gm, rz, str_, brec[:, cout:], rows)
    dzr = o_dzr.cpu()
    dtz = o_dtz.cpu()
    for nm, ref, og, ob, dx in (("3", ref3, o_g3, o_b3, dtz), ("r", refr, o_gr, o_brr, dzr[:, K * cout:])):
        check(k, "dgamma" + nm, og.cpu()[0], *ref["dgamma"])
        check(k, "dbeta" + nm, ob.cpu()[0], *ref["dbeta"])
        check(k, "dX" + nm, dx, *ref["dX"])
    dar, dab = R.tconv_input_grad(dtz, Wt, B, T, V)
    dy0 = o_dy0.cpu()
    check(k, "dy0", dy0, dar, dab)
    bw = check_records(k, "bw_rec", o_bw, B, cout, *R.g_records(dy0, dar, dab, ym, st0, R.groups(rows, T * V)), "", summed=True)
    ref0 = R.bn_bwd(dy0.double() * m0, ym, st0, bw, rows)
    check(k, "dgamma0", o_g0.cpu()[0], *ref0["dgamma"])
    check(k, "dbeta0", o_b0.cpu()[0], *ref0["dbeta"])
    gd = R.graph_dA(zr[:, :K * cout], ref0["dX"][0], ref0["dXmag"], A, imp, F, V, K, cout)
    check(k, "dZ", dzr[:, :K * cout], *gd["dZ"])
    check(k, "partial", o_pa.cpu().view(nda, K, V, V), *gd["partial"])
    for o in (o_x, o_zr, o_ym, o_ry, o_rr, o_tz, o_y0, o_r3, o_out, o_kv, o_br, o_dzr, o_dtz, o_g3, o_b3, o_gr, o_brr, o_g0, o_b0, o_dy0, o_bw, o_pa):
        assert o.guards_intact()
    # ---- the references compose to the block's gradient: float64 autograd with the same masks
    names = ("Wc", "bc", "g0", "b0", "Wt", "bt", "g3", "b3", "gr", "br")
    vals = (Wc, bc, bn0.gamma, bn0.beta, Wt, bt, bn3.gamma, bn3.beta, bnr.gamma, bnr.beta)
    P = {n: v.double().requires_grad_(True) for n, v in zip(names, vals)}
    Ai = (A.double() * imp.double()).requires_grad_(True)
    masks = (m0.double(), mout)
    outa, mid = R.block_torch(x.detach(), P, Ai, torch.ones_like(Ai), B, T, V, K, cout, masks)
    for t in mid.values():
        t.retain_grad()
    (outa * dout.double()).sum().backward()
    with torch.no_grad():
        f = block_by_references(x, {n: v.detach() for n, v in P.items()}, A.double(), imp.double(), B, T, V, K, cout, masks, dout.double())
    want = {"dz": mid["zr"].grad[:, :K * cout], "drz": mid["zr"].grad[:, K * cout:], "dAimp": Ai.grad, "dg0": P["g0"].grad, "db0": P["b0"].grad,
            "dg3": P["g3"].grad, "db3": P["b3"].grad, "dgr": P["gr"].grad, "dbr": P["br"].grad, "dtz": mid["tz"].grad, "dy0": mid["y0"].grad}
    for nm, w in want.items():
        assert float((f[nm] - w).abs().max()) <= 1e-9 * max(1.0, float(w.abs().max())), nm
