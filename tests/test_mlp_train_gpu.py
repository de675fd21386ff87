"""GPU: the train-mode pointwise MLP kernels of csrc/mlp_train.hip, each on its own through the C ABI, against float64.

Every reference is plain float64 torch on the CPU computed from the fp32 values the kernel read.  The ReLU masks are the kernel's own
masks exactly: the kernels decide with fmaf(z - mean, a, b) > 0 in fp32, and the sign of that equals the sign of
float32(z - mean).double() * a.double() + b.double() (a product of two fp32 numbers is exact in fp64 and the addition cannot change a
sign), so no element is left out of any comparison and nothing near the threshold is treated specially.

Tolerances are a-priori fp32 rounding bounds, |out - ref| <= MARGIN * bound elementwise, with
  * products (Z, dX, dW_part): (n + c) 2^-24 sum_i |a_i| |b_i|, n the length of the accumulation chain and c the roundings in front of
    the product, |a_i| / |b_i| the magnitudes those roundings are relative to (see CDZ, CACT below);
  * mean, invstd, a, running statistics: the fp32 roundings of their expressions plus the fp64 error of the sums behind them;
  * fp64-accumulated records (statistics partials, g partials, dgamma, dbeta): the fp32 rounding of the summands and of the stored
    result plus n 2^-53 sum |summand|.
MARGIN is the one constant of the file; NOTES.md ("Float64 tests of mlp_train.hip") holds the measured error / bound ratios.

Shapes: the row counts are those at which mt_grid and the kernels change behaviour (test_grid_rule_and_forms pins the rule); every
operand runs dense and as a column slice (ld = C + 3) of a buffer whose base lies one float past an aligned address; every output has
64 guard rows, the guard columns of the slice and guard records, pre-filled with a sentinel that must survive."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U64 = 2.0 ** -53
MARGIN = 4.0            # for what the bounds do not model (1 / sqrt, casts, second-order terms)
SENT = 7777.0
GUARD = 64
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))      # what the kernels' (float) cast of eps gives
MOM = float(torch.tensor(0.1, dtype=torch.float32))        # exactly representable: kernel and torch use the same momentum
NAN = float("nan")
# roundings in front of the dW / dX products: dz = a (g - c1 - ((z - mu) is) c2) -- z - mu, * is, * c2, g - c1, the second subtraction,
# a *, and the fp32 roundings of c1 and c2 themselves -- each relative to at most |a| (|g| + |c1| + |xhat c2|)
CDZ = 8
# act(x) = max(fmaf(x - mu, a, b), 0): the subtraction and the fma, relative to at most |x - mu| |a| + |b|
CACT = 2

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
            print("RATIO %-22s %-14s %.4g" % (k, o, r))


def call(name, *args):
    from mmego_amd import hip
    hip.call(name, *args)


# ---------------------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------------------
def mt_grid(rows):
    """mlp_train.hip mt_grid: (workgroups = partial records, rows per workgroup)."""
    tiles = (rows + 255) // 256
    tpw = -(-tiles // min(tiles, 256))
    return -(-tiles // tpw), tpw * 256


FORMS = {3: "ragged", 64: "ragged", 65: "ragged", 129: "ragged", 255: "ragged", 257: "ragged", 256: "FULL", 4096: "FULL",
         1920: "ragged", 66381: "ragged", 66560: "FULL", 1512: "ragged", 6912: "FULL", 4173: "ragged"}
NET_WIDTHS = [(6, 8), (8, 16), (16, 24), (6, 16), (16, 32), (32, 61), (28, 32), (31, 32), (32, 48), (48, 64)]
EDGE_WIDTHS = [(1, 1), (64, 64), (33, 31), (5, 64), (64, 3)]
SMALL_ROWS = [3, 64, 65, 129, 255, 257, 256, 4096, 1920]


def _cases():
    out = []
    for i, (ci, co) in enumerate(NET_WIDTHS + EDGE_WIDTHS):        # every width dense and sliced, paired with the row counts in turn
        out.append((SMALL_ROWS[i % 9], ci, co, bool(i & 1)))
        out.append((SMALL_ROWS[(i + 4) % 9], ci, co, not (i & 1)))
    out += [(66381, 33, 31, True), (66381, 48, 64, False), (66560, 64, 64, False), (66560, 6, 8, True)]
    return out


CASES = _cases()
case_id = lambda c: "%d-%dx%d-%s" % (c[0], c[1], c[2], "sliced" if c[3] else "dense")
cases = pytest.mark.parametrize("case", CASES, ids=case_id)


def test_grid_rule_and_forms(dev):
    """mmego_mlp_train_nblk against the Python copy of mt_grid, and the row counts of this file are the cases they claim to be."""
    from mmego_amd import hip
    for rows, form in FORMS.items():
        nblk, rpw = mt_grid(rows)
        assert hip.lib().mmego_mlp_train_nblk(rows) == nblk, rows
        assert (rows % rpw == 0) == (form == "FULL"), rows
        assert nblk * rpw >= rows > (nblk - 1) * rpw
    assert mt_grid(66381) == (130, 512) and 66381 - 129 * 512 == 256 + 77
    assert mt_grid(66560) == (130, 512) and mt_grid(4096) == (16, 256) and mt_grid(4173) == (17, 256) and mt_grid(257) == (2, 256)
    assert mt_grid(1920) == (8, 256) and mt_grid(1512) == (6, 256) and mt_grid(6912) == (27, 256)
    assert {c[0] for c in CASES} == set(SMALL_ROWS) | {66381, 66560}
    for w in NET_WIDTHS + EDGE_WIDTHS:
        assert {c[3] for c in CASES if c[1:3] == w} == {True, False}


# ---------------------------------------------------------------------------------------------------------------------------------
# device buffers: operands (dense / sliced, NaN around them) and outputs (sentinel around them)
# ---------------------------------------------------------------------------------------------------------------------------------
def d_mat(dev, t, sliced):
    """[rows][C] operand -> (device view, ld).  sliced: columns 0..C-1 of a [rows][C + 3] buffer that starts one element past an aligned
    address, NaN everywhere else."""
    rows, C = t.shape
    if not sliced:
        return t.to(dev).contiguous(), C
    ld = C + 3
    buf = torch.full((1 + rows * ld,), NAN, dtype=t.dtype, device=dev)
    v = buf[1:].view(rows, ld)[:, :C]
    v.copy_(t)
    return v, ld


def d_vec(dev, t, sliced):
    """A contiguous operand (weights, bias, gamma, state, records): dense, or one element past an aligned address."""
    flat = t.contiguous().view(-1)
    buf = torch.full((flat.numel() + 2,), NAN, dtype=t.dtype, device=dev)
    off = 1 if sliced else 0
    v = buf[off:off + flat.numel()]
    v.copy_(flat)
    return v


class Out:
    """An output [rows][C] with GUARD extra rows (and, sliced, three extra columns and a base one element past an aligned address),
    pre-filled with the sentinel.  strided=False: an output the ABI takes without a leading dimension."""

    def __init__(self, dev, rows, C, sliced=False, dtype=torch.float32, strided=True):
        self.rows, self.C = rows, C
        self.ld = C + 3 if (sliced and strided) else C
        self.off = 1 if sliced else 0
        self.buf = torch.full((self.off + (rows + GUARD) * self.ld,), SENT, dtype=dtype, device=dev)
        self.view = self.buf[self.off:].view(rows + GUARD, self.ld)[:rows, :C]

    def cpu(self):
        return self.view.cpu()

    def guards_intact(self):
        b = self.buf.clone()
        b[self.off:].view(self.rows + GUARD, self.ld)[:self.rows, :self.C] = SENT
        return bool((b == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def d_records(dev, rec, sliced=False):
    """Statistics records [nblk][2][C] (fp64) as a kernel reads them: [nblk][2][64], NaN in the unused columns and in two records behind
    the last (a record read past nblk, or a column past C, poisons the result)."""
    nblk, _, C = rec.shape
    full = torch.full((nblk + 2, 2, 64), NAN, dtype=torch.float64)
    full[:nblk, :, :C] = rec
    return d_vec(dev, full, sliced)


def gen_for(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def randn(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


def rand_state(g, C):
    """A sane BatchNorm state [4][C]: mean, invstd > 0, a = gamma invstd (either sign), b."""
    mean, invstd = randn(g, C, scale=0.3), torch.rand(C, generator=g) + 0.5
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    return torch.stack((mean, invstd, gamma * invstd, randn(g, C, scale=0.3)))


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def check(kernel, name, out, ref, bound, note=""):
    """|out - ref| <= MARGIN * bound elementwise (bound 0: equal), every element; records the largest error / bound ratio."""
    out, ref, bound = out.double().cpu(), ref.double(), bound.double().expand_as(ref)
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


def wg_sum(t, rows):
    """Sums of t [rows][...] over the rows of each workgroup -> [nblk][...]."""
    nblk, rpw = mt_grid(rows)
    pad = nblk * rpw - rows
    if pad:
        t = torch.cat((t, t.new_zeros((pad,) + tuple(t.shape[1:]))))
    return t.view(nblk, rpw, *t.shape[1:]).sum(1)


def wg_rows(rows):
    nblk, rpw = mt_grid(rows)
    return [min(rows, (j + 1) * rpw) - j * rpw for j in range(nblk)]


def dw_chain(n):
    """Longest accumulation chain of a dW_part element of a workgroup with n rows: the rows of group 0's tiles (tiles 0, 2, 4, ..: one
    MFMA accumulation each) plus the addition of group 1's accumulator."""
    return sum(min(64, n - 64 * t) for t in range(0, (n + 63) // 64, 2)) + 1


def bn_parts(z, st):
    """z [rows][C] fp32, st [4][C] fp32 as the kernel reads them -> the kernel's mask bn(z) > 0 exactly; bn(z), its magnitude
    |z - mean| |a| + |b|, |z - mean| |a| and xhat = (z - mean) invstd in fp64."""
    mean, istd, a, b = st[0], st[1], st[2], st[3]
    mask = ((z - mean).double() * a.double() + b.double()) > 0          # fp32 subtraction, the rest exact
    d = z.double() - mean.double()
    da = d.abs() * a.abs().double()
    return mask, d * a.double() + b.double(), da + b.abs().double(), da, d * istd.double()


def ref_product(xact, xmag, cx, W, bias):
    """Z = xact W^T (+ bias) in fp64 and its bound: K accumulated terms, cx roundings in front, one for the bias."""
    Wd = W.double()
    z, zm, c = xact @ Wd.t(), xmag @ Wd.abs().t(), cx
    if bias is not None:
        z, zm, c = z + bias.double(), zm + bias.abs().double(), c + 1
    return z, (W.shape[1] + c) * U32 * zm


def ref_stats(z, gamma, beta, rm0, rv0):
    """BatchNorm state and torch's running-statistics update from z (fp32, the kernel's own) in fp64, with bounds.
    mean, invstd: one fp32 rounding of the fp64 value; a = gamma invstd: two; b = beta: none.  Running statistics: 1 - momentum, its
    product with the old value, the rounding of the statistic, its product with the momentum and the sum.  Behind each, the fp64 error
    of the N-term sums (and of the cancellation in var = S2 / N - mean^2)."""
    zd = z.double()
    N = zd.shape[0]
    m = zd.mean(0)
    S2 = (zd * zd).sum(0) / N
    var = (S2 - m * m).clamp_min(0.0)
    istd = 1.0 / torch.sqrt(var + EPS32)
    e_m = (N + 1) * U64 * zd.abs().sum(0) / N
    e_var = (N + 3) * U64 * (S2 + m * m)
    b_istd = U32 * istd + 0.5 * istd ** 3 * e_var
    a = gamma.double() * istd
    state = torch.stack((m, istd, a, beta.double()))
    bound = torch.stack((U32 * m.abs() + e_m, b_istd, gamma.abs().double() * b_istd + U32 * a.abs(), torch.zeros_like(m)))
    rm, rv = rm0.double().clone(), rv0.double().clone()
    F.batch_norm(zd, rm, rv, None, None, True, MOM, EPS32)                # torch's own update
    unb = var * N / (N - 1)
    b_rm = U32 * (2 * ((1 - MOM) * rm0.double()).abs() + 2 * (MOM * m).abs() + rm.abs()) + MOM * e_m
    b_rv = U32 * (2 * ((1 - MOM) * rv0.double()).abs() + 2 * MOM * unb + rv.abs()) + MOM * e_var * N / (N - 1)
    return state, bound, rm, b_rm, rv, b_rv


def check_stats(kernel, z_cpu, gamma, beta, rm0, rv0, o_state, o_rm, o_rv, note):
    """state and running statistics.  The running statistics started from non-trivial values and every workgroup finalizes: a second
    update (or none) is off by momentum |statistic - old value|, ~1e-2 against a bound of ~1e-7 -- they were updated exactly once."""
    state, b_state, rm, b_rm, rv, b_rv = ref_stats(z_cpu, gamma, beta, rm0, rv0)
    got = o_state.cpu()
    for q, nm in enumerate(("mean", "invstd", "a", "b")):
        check(kernel, "state." + nm, got[q], state[q], b_state[q], note)
    check(kernel, "running_mean", o_rm.cpu()[0], rm, b_rm, note)
    check(kernel, "running_var", o_rv.cpu()[0], rv, b_rv, note)
    for o in (o_state, o_rm, o_rv):
        assert o.guards_intact(), (kernel, note)
    return got


def check_records(kernel, name, o_part, rows, s1, b1, s2, b2, C, note):
    """Partial records [nblk][2][64]: per workgroup (pins the rows a workgroup owns) and summed; zero in the unused columns; guard
    records untouched."""
    nblk, _ = mt_grid(rows)
    got = o_part.cpu().view(nblk, 2, 64)
    check(kernel, name + ".s1", got[:, 0, :C], s1, b1, note)
    check(kernel, name + ".s2", got[:, 1, :C], s2, b2, note)
    check(kernel, name + ".s1 summed", got[:, 0, :C].sum(0), s1.sum(0), b1.sum(0), note)
    check(kernel, name + ".s2 summed", got[:, 1, :C].sum(0), s2.sum(0), b2.sum(0), note)
    assert float(got[:, :, C:].abs().max()) == 0.0 if C < 64 else True, (kernel, name, note)
    assert o_part.guards_intact(), (kernel, name, note)


def upper(ref, bound):
    """An a-priori ceiling of |out| for an output that has just passed check(out, ref, bound): magnitudes for the bounds of what a
    kernel derives from that output come from here, never from the output itself (a wrong output cannot widen its own tolerance)."""
    return ref.abs() + MARGIN * bound


def sum_records(zd, rows, zmax):
    """(sum z, sum z^2) per workgroup of z (the kernel's own Z as the issue prescribes; fp64 copy of fp32 values: the squares are
    exact) and the fp64 accumulation bounds, whose magnitudes are zmax = upper(...) of the float64 reference of Z."""
    n = torch.tensor(wg_rows(rows), dtype=torch.float64).view(-1, 1)
    s1, s2 = wg_sum(zd, rows), wg_sum(zd * zd, rows)
    return s1, n * U64 * wg_sum(zmax, rows), s2, n * U64 * wg_sum(zmax * zmax, rows)


def gprev_records(dx, ref_dx, mask_in, xhat_in, rows):
    """(sum g', sum g' xhat') per workgroup with g' = dX . [act(xin) > 0] from the kernel's own fp32 dX (what the kernel sums; dX was
    held to float64 just before) and their bounds as in ref_g_records, the magnitudes from the float64 reference of dX."""
    gp = dx.double() * mask_in
    gmax = upper(*ref_dx) * mask_in
    n = torch.tensor(wg_rows(rows), dtype=torch.float64).view(-1, 1)
    a1, a2 = wg_sum(gmax, rows), wg_sum(gmax * xhat_in.abs(), rows)
    return wg_sum(gp, rows), n * U64 * a1, wg_sum(gp * xhat_in, rows), 2 * U32 * a2 + n * U64 * a2


# ---------------------------------------------------------------------------------------------------------------------------------
# mlp_fwd_layer / mlp_fwd_layer_n
# ---------------------------------------------------------------------------------------------------------------------------------
@cases
def test_fwd_layer_identity_input(dev, case):
    """Z = X W^T + b and the (sum z, sum z^2) records of the kernel's own Z, with and without a bias."""
    rows, Cin, Cout, sliced = case
    g = gen_for(1, *case)
    x, W, b = randn(g, rows, Cin, scale=0.8, shift=0.1), randn(g, Cout, Cin, scale=0.5), randn(g, Cout, scale=0.3)
    nblk, _ = mt_grid(rows)
    dx, ldx = d_mat(dev, x, sliced)
    for bias in (b, None):
        oz, op = Out(dev, rows, Cout, sliced), Out(dev, nblk, 128, sliced, torch.float64, strided=False)
        call("mlp_fwd_layer", dx, ldx, rows, Cin, None, None, None, 0.0, None, None, 0.0, None, d_vec(dev, W, sliced),
             None if bias is None else d_vec(dev, bias, sliced), Cout, oz.view, oz.ld, op.view)
        note = case_id(case) + (" bias" if bias is not None else " no bias")
        z, bz = ref_product(x.double(), x.abs().double(), 0, W, bias)
        check("mlp_fwd_layer", "Z", oz.cpu(), z, bz, note)
        assert oz.guards_intact(), note
        check_records("mlp_fwd_layer", "out_part", op, rows, *sum_records(oz.cpu().double(), rows, upper(z, bz)), Cout, note)


def _fwd_pair(dev, case, in_nblk=None):
    """Two chained calls: z1 = x W1^T + b1, then z2 = relu(bn(z1)) W2^T + b2 with bn finalized from the first call's records
    (in_nblk: from in_nblk hand-made records of the same column sums through mlp_fwd_layer_n)."""
    rows, Cin, Cout, sliced = case
    g = gen_for(2, *case)
    x, W1, b1 = randn(g, rows, Cin, scale=0.8, shift=0.1), randn(g, Cout, Cin, scale=0.5), randn(g, Cout, scale=0.3)
    C2 = Cin                                                             # the second layer: Cout -> Cin channels
    W2, b2 = randn(g, C2, Cout, scale=0.5), randn(g, C2, scale=0.3)
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5) * torch.where(torch.rand(Cout, generator=g) < 0.25, -1.0, 1.0), randn(g, Cout, scale=0.3)
    rm0, rv0 = randn(g, Cout, scale=0.4), torch.rand(Cout, generator=g) + 0.5
    nblk, _ = mt_grid(rows)
    dx, ldx = d_mat(dev, x, sliced)
    oz1, op1 = Out(dev, rows, Cout, sliced), Out(dev, nblk, 128, sliced, torch.float64, strided=False)
    call("mlp_fwd_layer", dx, ldx, rows, Cin, None, None, None, 0.0, None, None, 0.0, None, d_vec(dev, W1, sliced), d_vec(dev, b1, sliced),
         Cout, oz1.view, oz1.ld, op1.view)
    z1 = oz1.cpu()
    o_state = Out(dev, 4, Cout, sliced, strided=False)
    o_rm, o_rv = Out(dev, 1, Cout, sliced, strided=False), Out(dev, 1, Cout, sliced, strided=False)
    o_rm.view.copy_(rm0.view(1, -1))
    o_rv.view.copy_(rv0.view(1, -1))
    oz2, op2 = Out(dev, rows, C2, sliced), Out(dev, nblk, 128, sliced, torch.float64, strided=False)
    tail = (d_vec(dev, gamma, sliced), d_vec(dev, beta, sliced), EPS, o_rm.view, o_rv.view, MOM, o_state.view, d_vec(dev, W2, sliced),
            d_vec(dev, b2, sliced), C2, oz2.view, oz2.ld, op2.view)
    if in_nblk is None:
        kernel, note = "mlp_fwd_layer", case_id(case) + " in_part"
        call("mlp_fwd_layer", oz1.view, oz1.ld, rows, Cout, op1.view, *tail)
    else:
        kernel, note = "mlp_fwd_layer_n", case_id(case) + " in_nblk %d" % in_nblk
        z1d = z1.double()
        rec = torch.stack([torch.stack((c.sum(0), (c * c).sum(0))) for c in torch.tensor_split(z1d, in_nblk)])     # empty chunks: zeros
        call("mlp_fwd_layer_n", oz1.view, oz1.ld, rows, Cout, d_records(dev, rec, sliced), in_nblk, *tail)
    st = check_stats(kernel, z1, gamma, beta, rm0, rv0, o_state, o_rm, o_rv, note)
    mask, val, mag, _, _ = bn_parts(z1, st)                              # with the state's fp32 values
    z2, bz2 = ref_product(mask * val, mask * mag, CACT, W2, b2)
    check(kernel, "Z (act input)", oz2.cpu(), z2, bz2, note)
    assert oz2.guards_intact() and oz1.guards_intact(), note
    check_records(kernel, "out_part", op2, rows, *sum_records(oz2.cpu().double(), rows, upper(z2, bz2)), C2, note)
    return oz2.cpu(), st


@cases
def test_fwd_layer_with_in_part(dev, case):
    """The second of two chained calls: in_state from the fp64 statistics of the first Z, running statistics like torch (updated once),
    Z = relu(bn(z1)) W^T + b with the state's fp32 values."""
    _fwd_pair(dev, case)


@pytest.mark.parametrize("case,in_nblk", [((3, 6, 8, False), 7), ((257, 33, 31, True), 1), ((257, 33, 31, True), 129), ((1920, 28, 32, False), 7),
                                          ((1920, 28, 32, True), 1024), ((4096, 64, 64, False), 129), ((66381, 48, 64, False), 1024),
                                          ((66381, 33, 31, True), 1)],
                         ids=lambda v: case_id(v) if isinstance(v, tuple) else "n%d" % v)
def test_fwd_layer_n(dev, case, in_nblk):
    """mlp_fwd_layer_n with the records re-cut by hand into 1, 7, 129 and 1024 records (same column sums, zeros where a record has no
    rows): the same state, running statistics and Z as mlp_fwd_layer, to the same bounds."""
    _fwd_pair(dev, case, in_nblk)


# ---------------------------------------------------------------------------------------------------------------------------------
# mlp_bn_act / mlp_bn_bwd_reduce
# ---------------------------------------------------------------------------------------------------------------------------------
@cases
def test_bn_act(dev, case):
    """Y = relu(bn(Z)), state and running statistics from records of Z (channels: the case's Cout)."""
    rows, _, C, sliced = case
    g = gen_for(3, *case)
    z = randn(g, rows, C, scale=1.1, shift=0.2)
    gamma, beta = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0), randn(g, C, scale=0.3)
    rm0, rv0 = randn(g, C, scale=0.4), torch.rand(C, generator=g) + 0.5
    zd = z.double()
    rec = torch.stack((wg_sum(zd, rows), wg_sum(zd * zd, rows)), 1)
    dz, ldz = d_mat(dev, z, sliced)
    oy, o_state = Out(dev, rows, C, sliced), Out(dev, 4, C, sliced, strided=False)
    o_rm, o_rv = Out(dev, 1, C, sliced, strided=False), Out(dev, 1, C, sliced, strided=False)
    o_rm.view.copy_(rm0.view(1, -1))
    o_rv.view.copy_(rv0.view(1, -1))
    call("mlp_bn_act", dz, ldz, rows, C, d_records(dev, rec, sliced), d_vec(dev, gamma, sliced), d_vec(dev, beta, sliced), EPS, o_rm.view,
         o_rv.view, MOM, o_state.view, oy.view, oy.ld)
    note = case_id(case)
    st = check_stats("mlp_bn_act", z, gamma, beta, rm0, rv0, o_state, o_rm, o_rv, note)
    mask, val, mag, da, _ = bn_parts(z, st)
    check("mlp_bn_act", "Y", oy.cpu(), mask * val, mask * U32 * (da + mag), note)          # the subtraction, then the fma
    assert oy.guards_intact(), note


def ref_g_records(dy, z, st, rows, mask=None):
    """g = dy . [bn(z) > 0]; (sum g, sum g xhat) per workgroup with bounds: the summands of s1 are exact, those of s2 carry the two fp32
    roundings of xhat = (z - mean) invstd; both accumulate in fp64.  mask: given instead of derived (see ref_bwd)."""
    xhat = bn_parts(z, st)[4]
    if mask is None:
        mask = bn_parts(z, st)[0]
    gm = dy.double() * mask
    n = torch.tensor(wg_rows(rows), dtype=torch.float64).view(-1, 1)
    s1, s2 = wg_sum(gm, rows), wg_sum(gm * xhat, rows)
    a1, a2 = wg_sum(gm.abs(), rows), wg_sum((gm * xhat).abs(), rows)
    return s1, n * U64 * a1, s2, 2 * U32 * a2 + n * U64 * a2


@cases
def test_bn_bwd_reduce(dev, case):
    """part = (sum g, sum g xhat) per workgroup against the masked fp64 sums."""
    rows, _, C, sliced = case
    g = gen_for(4, *case)
    z, dy, st = randn(g, rows, C, scale=1.1, shift=0.2), randn(g, rows, C), rand_state(g, C)
    nblk, _ = mt_grid(rows)
    (dz, ldz), (ddy, lddy) = d_mat(dev, z, sliced), d_mat(dev, dy, sliced)
    op = Out(dev, nblk, 128, sliced, torch.float64, strided=False)
    call("mlp_bn_bwd_reduce", ddy, lddy, dz, ldz, rows, C, d_vec(dev, st, sliced), op.view)
    check_records("mlp_bn_bwd_reduce", "part", op, rows, *ref_g_records(dy, z, st, rows), C, case_id(case))


# ---------------------------------------------------------------------------------------------------------------------------------
# mlp_bwd_layer
# ---------------------------------------------------------------------------------------------------------------------------------
def ref_bwd(dy, z, st, rec, xin, in_st, W, rows, masks=None):
    """fp64 reference of one backward layer from the fp32 values the kernel reads; rec [nblk][2][Cout] are the (sum g, sum g xhat) records.
    -> dict of (reference, bound).  masks = (this layer's, the layer below's or None): given instead of derived from z and st (the
    chain test runs this same function on float64 operands with the device's masks, against autograd)."""
    mask, _, _, _, xhat = bn_parts(z, st)
    if masks is not None:
        mask = masks[0]
    a = st[2].double()
    gm = dy.double() * mask
    S1, S2 = rec[:, 0].sum(0), rec[:, 1].sum(0)
    eS = rec.shape[0] * U64
    c1, c2 = S1 / rows, S2 / rows
    dz = a * (gm - c1 - xhat * c2)
    dzm = a.abs() * (gm.abs() + c1.abs() + (xhat * c2).abs())
    Wd = W.double()
    Cout, Cin = W.shape
    out = {"dbeta": (S1, U32 * S1.abs() + eS * rec[:, 0].abs().sum(0)), "dgamma": (S2, U32 * S2.abs() + eS * rec[:, 1].abs().sum(0)),
           "dX": (dz @ Wd, (Cout + CDZ) * U32 * (dzm @ Wd.abs()))}
    if in_st is not None:
        mask_in, val, mag, _, xhat_in = bn_parts(xin, in_st)
        if masks is not None:
            mask_in = masks[1]
        act, am, cx = mask_in * val, mask_in * mag, CACT
        out["mask_in"], out["xhat_in"] = mask_in, xhat_in
    else:
        act, am, cx = xin.double(), xin.abs().double(), 0
    nblk, rpw = mt_grid(rows)
    pad = nblk * rpw - rows
    P = lambda t: torch.cat((t, t.new_zeros(pad, t.shape[1]))).view(nblk, rpw, -1) if pad else t.view(nblk, rpw, -1)
    dw = torch.bmm(P(dz).transpose(1, 2), P(act))
    dwm = torch.bmm(P(dzm).transpose(1, 2), P(am))
    n = torch.tensor([dw_chain(r) for r in wg_rows(rows)], dtype=torch.float64).view(-1, 1, 1)
    out["dW_part"] = (dw, (n + CDZ + cx) * U32 * dwm)
    return out


def check_dw_part(kernel, o_dw, ref, rows, Cout, Cin, note):
    nblk, _ = mt_grid(rows)
    got = o_dw.cpu().view(nblk, 64, 64)
    check(kernel, "dW_part", got[:, :Cout, :Cin], ref[0], ref[1], note)
    check(kernel, "dW_part summed", got[:, :Cout, :Cin].double().sum(0), ref[0].sum(0), ref[1].sum(0), note)
    pad = got.clone()
    pad[:, :Cout, :Cin] = 0.0
    assert float(pad.abs().max()) == 0.0, (kernel, "dW_part padding", note)
    assert o_dw.guards_intact(), (kernel, "dW_part guard records", note)


def bwd_inputs(g, rows, Cin, Cout, with_in_state):
    z, dy, st = randn(g, rows, Cout, scale=1.1, shift=0.2), randn(g, rows, Cout), rand_state(g, Cout)
    xin = randn(g, rows, Cin, scale=0.9, shift=0.1)
    W = randn(g, Cout, Cin, scale=0.5)
    s1, _, s2, _ = ref_g_records(dy, z, st, rows)
    return z, dy, st, xin, (rand_state(g, Cin) if with_in_state else None), W, torch.stack((s1, s2), 1)


@cases
def test_bwd_layer_top(dev, case):
    """A top layer: in_state and gprev_part given.  dgamma, dbeta, dX, the dW_part records (each against its own workgroup's rows, and
    summed) and gprev_part -- the latter against the masked fp64 sums of the kernel's own dX (checked just before), within a bound
    whose magnitudes are the float64 reference's."""
    rows, Cin, Cout, sliced = case
    g = gen_for(5, *case)
    z, dy, st, xin, in_st, W, rec = bwd_inputs(g, rows, Cin, Cout, True)
    nblk, _ = mt_grid(rows)
    (dz, ldz), (ddy, lddy), (dxin, ldxin) = d_mat(dev, z, sliced), d_mat(dev, dy, sliced), d_mat(dev, xin, sliced)
    o_dg, o_db = Out(dev, 1, Cout, sliced, strided=False), Out(dev, 1, Cout, sliced, strided=False)
    o_dx, o_gp = Out(dev, rows, Cin, sliced), Out(dev, nblk, 128, sliced, torch.float64, strided=False)
    o_dw = Out(dev, nblk, 4096, sliced, strided=False)
    call("mlp_bwd_layer", ddy, lddy, dz, ldz, rows, Cout, d_vec(dev, st, sliced), d_records(dev, rec, sliced), o_dg.view, o_db.view, dxin, ldxin,
         Cin, d_vec(dev, in_st, sliced), d_vec(dev, W, sliced), o_dx.view, o_dx.ld, o_gp.view, o_dw.view)
    note, k = case_id(case), "mlp_bwd_layer"
    ref = ref_bwd(dy, z, st, rec, xin, in_st, W, rows)
    check(k, "dgamma", o_dg.cpu()[0], *ref["dgamma"], note)
    check(k, "dbeta", o_db.cpu()[0], *ref["dbeta"], note)
    check(k, "dX", o_dx.cpu(), *ref["dX"], note)
    assert o_dg.guards_intact() and o_db.guards_intact() and o_dx.guards_intact(), note
    check_dw_part(k, o_dw, ref["dW_part"], rows, Cout, Cin, note)
    check_records(k, "gprev_part", o_gp, rows, *gprev_records(o_dx.cpu(), ref["dX"], ref["mask_in"], ref["xhat_in"], rows), Cin, note)


@cases
def test_bwd_layer_first(dev, case):
    """A first layer (in_state = NULL, gprev_part = NULL): with dX, and with dX = NULL -- then the dW_part records, dgamma and dbeta are
    bit-identical to the first form's and no input gradient is written."""
    rows, Cin, Cout, sliced = case
    g = gen_for(6, *case)
    z, dy, st, xin, _, W, rec = bwd_inputs(g, rows, Cin, Cout, False)
    nblk, _ = mt_grid(rows)
    (dz, ldz), (ddy, lddy), (dxin, ldxin) = d_mat(dev, z, sliced), d_mat(dev, dy, sliced), d_mat(dev, xin, sliced)
    ref = ref_bwd(dy, z, st, rec, xin, None, W, rows)
    note, k = case_id(case), "mlp_bwd_layer"
    res = []
    for want_dx in (True, False):
        o_dg, o_db = Out(dev, 1, Cout, sliced, strided=False), Out(dev, 1, Cout, sliced, strided=False)
        o_dx, o_dw = Out(dev, rows, Cin, sliced), Out(dev, nblk, 4096, sliced, strided=False)
        call("mlp_bwd_layer", ddy, lddy, dz, ldz, rows, Cout, d_vec(dev, st, sliced), d_records(dev, rec, sliced), o_dg.view, o_db.view, dxin,
             ldxin, Cin, None, d_vec(dev, W, sliced), o_dx.view if want_dx else None, o_dx.ld if want_dx else 0, None, o_dw.view)
        check(k, "dgamma", o_dg.cpu()[0], *ref["dgamma"], note)
        check(k, "dbeta", o_db.cpu()[0], *ref["dbeta"], note)
        if want_dx:
            check(k, "dX (first layer)", o_dx.cpu(), *ref["dX"], note)
            assert o_dx.guards_intact(), note
        else:
            assert o_dx.untouched(), note
        assert o_dg.guards_intact() and o_db.guards_intact(), note
        check_dw_part(k, o_dw, ref["dW_part"], rows, Cout, Cin, note + (" dX" if want_dx else " dX=NULL"))
        res.append((o_dg.cpu(), o_db.cpu(), o_dw.cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b), (note, "changed by the absence of dX")


@pytest.mark.parametrize("rows,D,Cout,sliced", [(1512, 25, 32, False), (1512, 0, 16, True), (6912, 25, 32, True), (6912, 0, 16, False)])
def test_bwd_layer_gather(dev, rows, D, Cout, sliced):
    """mlp_bwd_layer_gather against mlp_bwd_layer fed the gathered tensor cat(anchor, xyz - anchor, features): the operand values are the
    same either way (xyz - anchor is one fp32 subtraction in torch as in the kernel) and so is every summation order: bit-equal dX,
    dgamma, dbeta and dW_part.  1512 rows: both launches take their clamped forms; 6912: the plain launch takes the FULL form."""
    N, Cin = 128, 6 + D
    Fn = rows // 216
    g = gen_for(7, rows, D)
    feats = randn(g, Fn * N, 3 + D, scale=0.7)
    anchors = randn(g, 27, 3, scale=0.5)
    gidx = torch.randint(0, N, (rows,), generator=g)
    r = torch.arange(rows)
    src = feats[(r // 216) * N + gidx]
    an = anchors[(r % 216) // 8]
    xin = torch.cat((an, src[:, :3] - an, src[:, 3:]), 1)
    z, dy, st = randn(g, rows, Cout, scale=1.1, shift=0.2), randn(g, rows, Cout), rand_state(g, Cout)
    W = randn(g, Cout, Cin, scale=0.5)
    s1, _, s2, _ = ref_g_records(dy, z, st, rows)
    rec = torch.stack((s1, s2), 1)
    nblk, _ = mt_grid(rows)
    (dz, ldz), (ddy, lddy), (dxin, ldxin), (dfe, ldf) = d_mat(dev, z, sliced), d_mat(dev, dy, sliced), d_mat(dev, xin, sliced), d_mat(dev, feats, sliced)
    res = []
    for gather in (False, True):
        o_dg, o_db = Out(dev, 1, Cout, sliced, strided=False), Out(dev, 1, Cout, sliced, strided=False)
        o_dx, o_dw = Out(dev, rows, Cin, sliced), Out(dev, nblk, 4096, sliced, strided=False)
        head = (ddy, lddy, dz, ldz, rows, Cout, d_vec(dev, st, sliced), d_records(dev, rec, sliced), o_dg.view, o_db.view)
        if gather:
            call("mlp_bwd_layer_gather", *head, gidx.to(dev), dfe, ldf, d_vec(dev, anchors, sliced), N, D, d_vec(dev, W, sliced), o_dx.view,
                 o_dx.ld, o_dw.view)
        else:
            call("mlp_bwd_layer", *head, dxin, ldxin, Cin, None, d_vec(dev, W, sliced), o_dx.view, o_dx.ld, None, o_dw.view)
        for o in (o_dg, o_db, o_dx, o_dw):
            assert o.guards_intact(), (rows, D, gather)
        res.append((o_dg.cpu(), o_db.cpu(), o_dx.cpu(), o_dw.cpu()))
    for nm, a, b in zip(("dgamma", "dbeta", "dX", "dW_part"), *res):
        assert torch.equal(a, b), (rows, D, nm, float((a - b).abs().max()))
    ref = ref_bwd(dy, z, st, rec, xin, None, W, rows)                      # and the pair is not wrong together
    check("mlp_bwd_layer_gather", "dX", res[1][2], *ref["dX"], "%d D=%d" % (rows, D))
    check("mlp_bwd_layer_gather", "dW_part", res[1][3].view(nblk, 64, 64)[:, :Cout, :Cin], *ref["dW_part"], "%d D=%d" % (rows, D))


# ---------------------------------------------------------------------------------------------------------------------------------
# mlp_dw_reduce
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlayers,rows", [(1, 256), (2, 4096), (3, 66381), (3, 256), (1, 66381)])
def test_dw_reduce(dev, nlayers, rows):
    """dW_l = sum of the nblk (1, 16, 130) partial records in fp64, within one ulp of part.double().sum(0).float(); nothing outside
    Cout x Cin is read (NaN there and in the records behind nblk) or written."""
    nblk, _ = mt_grid(rows)
    assert nblk == {256: 1, 4096: 16, 66381: 130}[rows]
    g = gen_for(8, nlayers, rows)
    dims = [(61, 32), (3, 64), (64, 33)][:nlayers]
    args, outs, refs = [], [], []
    for Cout, Cin in dims:
        part = torch.full((nblk + 2, 64, 64), NAN)
        part[:nblk, :Cout, :Cin] = randn(g, nblk, Cout, Cin)
        o = Out(dev, 1, Cout * Cin, strided=False)
        args += [part.to(dev), o.view, Cout, Cin]
        outs.append(o)
        refs.append(part[:nblk, :Cout, :Cin].double().sum(0).float().view(-1))
    args += [None, None, 0, 0] * (3 - nlayers)
    call("mlp_dw_reduce", rows, nlayers, *args)
    for o, ref in zip(outs, refs):
        got = o.cpu()[0]
        ulp = torch.nextafter(ref.abs(), torch.tensor(float("inf"))) - ref.abs()
        worst = float(((got - ref).abs() / ulp).max())                     # (one ulp: MARGIN does not apply)
        RATIOS[("mlp_dw_reduce", "dW (ulps)")] = max(RATIOS.get(("mlp_dw_reduce", "dW (ulps)"), 0.0), worst)
        assert worst <= 1.0, (nlayers, nblk, worst)
        assert o.guards_intact()


# ---------------------------------------------------------------------------------------------------------------------------------
# the two code forms on the rows they share
# ---------------------------------------------------------------------------------------------------------------------------------
def test_forms_agree_forward(dev):
    """mlp_fwd_layer with an identity input is row-independent: rows 0..4095 of a 4096-row launch (FULL form) and of a 4173-row launch
    (every workgroup in the ragged form) are bit-equal, and so are the records of the sixteen workgroups they share."""
    g = gen_for(9)
    Cin, Cout = 31, 48
    x, W, b = randn(g, 4173, Cin, scale=0.8), randn(g, Cout, Cin, scale=0.5), randn(g, Cout, scale=0.3)
    res = []
    for rows in (4096, 4173):
        nblk, _ = mt_grid(rows)
        oz, op = Out(dev, rows, Cout), Out(dev, nblk, 128, False, torch.float64)
        call("mlp_fwd_layer", x[:rows].to(dev), Cin, rows, Cin, None, None, None, 0.0, None, None, 0.0, None, W.to(dev), b.to(dev), Cout, oz.view,
             oz.ld, op.view)
        assert oz.guards_intact() and op.guards_intact()
        res.append((oz.cpu()[:4096], op.cpu()[:16]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_forms_agree_backward(dev):
    """mlp_bwd_layer with an all-zero g_part has c1 = c2 = 0, so dX is row-independent: the same two launches give bit-equal dX on the
    shared rows and bit-equal dW_part / gprev_part records 0..15."""
    g = gen_for(10)
    Cin, Cout = 33, 61
    z, dy, st, xin, in_st, W, _ = bwd_inputs(g, 4173, Cin, Cout, True)
    res = []
    for rows in (4096, 4173):
        nblk, _ = mt_grid(rows)
        o_dg, o_db = Out(dev, 1, Cout), Out(dev, 1, Cout)
        o_dx, o_gp, o_dw = Out(dev, rows, Cin), Out(dev, nblk, 128, False, torch.float64), Out(dev, nblk, 4096)
        call("mlp_bwd_layer", dy[:rows].to(dev), Cout, z[:rows].to(dev), Cout, rows, Cout, st.to(dev), d_records(dev, torch.zeros(nblk, 2, Cout, dtype=torch.float64)),
             o_dg.view, o_db.view, xin[:rows].to(dev), Cin, Cin, in_st.to(dev), W.to(dev), o_dx.view, o_dx.ld, o_gp.view, o_dw.view)
        for o in (o_dg, o_db, o_dx, o_gp, o_dw):
            assert o.guards_intact()
        assert float(o_dg.cpu().abs().max()) == 0.0 and float(o_db.cpu().abs().max()) == 0.0
        res.append((o_dx.cpu()[:4096], o_dw.cpu()[:16], o_gp.cpu()[:16]))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][0].abs().max()) > 0.1


# ---------------------------------------------------------------------------------------------------------------------------------
# one chain, end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _block_by_references(x, Ws, bs, gammas, betas, masks, dy, rows):
    """The block's gradients computed by the very reference functions the kernels are held to -- ref_product, ref_stats and bn_parts
    forward; ref_g_records, ref_bwd and gprev_records backward, chained as the launches are chained -- on float64 operands (every
    "fp32" step of theirs is then exact) with the given ReLU masks -> dW0..2, dgamma0..2, dbeta0..2, dx."""
    acts, zs, sts = [x], [], []
    for W, b, ga, be, M in zip(Ws, bs, gammas, betas, masks):
        zs.append(ref_product(acts[-1], acts[-1].abs(), 0, W, b)[0])
        sts.append(ref_stats(zs[-1], ga, be, torch.zeros_like(ga), torch.ones_like(ga))[0])
        acts.append(M * bn_parts(zs[-1], sts[-1])[1])
    s1, _, s2, _ = ref_g_records(dy, zs[2], sts[2], rows, masks[2])
    out, d = {}, dy
    for i in (2, 1, 0):
        r = ref_bwd(d, zs[i], sts[i], torch.stack((s1, s2), 1), zs[i - 1] if i else x, sts[i - 1] if i else None, Ws[i], rows,
                    (masks[i], masks[i - 1] if i else None))
        out["dW%d" % i], out["dgamma%d" % i], out["dbeta%d" % i], d = r["dW_part"][0].sum(0), r["dgamma"][0], r["dbeta"][0], r["dX"][0]
        if i:
            s1, _, s2, _ = gprev_records(d, r["dX"], r["mask_in"], r["xhat_in"], rows)
    out["dx"] = d
    return out


@pytest.mark.parametrize("dims", [(6, 16, 32, 61), (28, 32, 48, 64)], ids=lambda d: "x".join(map(str, d)))
def test_chain_end_to_end(dev, dims):
    """Three stages forward, mlp_bn_act, mlp_bn_bwd_reduce, three mlp_bwd_layer and mlp_dw_reduce at 1920 rows (ragged), issued exactly
    as blocks._mlp3_forward_fused / _mlp3_backward_fused issue them, every buffer handed from launch to launch on the device.

    Tolerance: the STAGE-WISE check repeated per stage (not propagated bounds).  Every launch's outputs are held to the fp64 formula of
    that launch fed the device's own inputs of that launch (the z_i, state_i, records and dy_i the chain produced), with the derived
    bounds of the single-kernel tests; the ReLU masks come from the device's own z_i and state_i by the sign identity.  The device's
    dW, dgamma, dbeta and input gradient are thus held to ref_bwd stage by stage, not to autograd directly; what ties the two is the
    last part of the test: the same reference functions (ref_product, ref_stats, ref_g_records, ref_bwd, gprev_records -- not a
    restatement of them), chained on float64 operands with those same masks, reproduce fp64 autograd of the block, each ReLU written
    as a multiplication with the mask, to 1e-9 of the largest element (fp64 summation error of 1920 rows is ~1e-13).  An error
    shared by a kernel and its reference would fail there."""
    rows = 1920
    nblk, _ = mt_grid(rows)
    g = gen_for(11, *dims)
    x = randn(g, rows, dims[0], scale=0.8, shift=0.1)
    Ws = [randn(g, dims[i + 1], dims[i], scale=0.5) for i in range(3)]
    bs = [randn(g, dims[i + 1], scale=0.3) for i in range(3)]
    gammas = [torch.rand(dims[i + 1], generator=g) + 0.5 for i in range(3)]
    betas = [randn(g, dims[i + 1], scale=0.3) for i in range(3)]
    rm0 = [randn(g, dims[i + 1], scale=0.4) for i in range(3)]
    rv0 = [torch.rand(dims[i + 1], generator=g) + 0.5 for i in range(3)]
    dy3 = randn(g, rows, dims[3])
    D = lambda t: t.to(dev)
    dW_, db_, dga_, dbe_ = [D(t) for t in Ws], [D(t) for t in bs], [D(t) for t in gammas], [D(t) for t in betas]
    oz = [Out(dev, rows, dims[i + 1]) for i in range(3)]
    osp = [Out(dev, nblk, 128, False, torch.float64) for _ in range(3)]
    ost = [Out(dev, 4, dims[i + 1]) for i in range(3)]
    orm, orv = [Out(dev, 1, dims[i + 1]) for i in range(3)], [Out(dev, 1, dims[i + 1]) for i in range(3)]
    for i in range(3):
        orm[i].view.copy_(rm0[i].view(1, -1))
        orv[i].view.copy_(rv0[i].view(1, -1))
    oy = Out(dev, rows, dims[3])
    dxd = D(x)
    # forward, as _mlp3_forward_fused
    call("mlp_fwd_layer", dxd, dims[0], rows, dims[0], None, None, None, 0.0, None, None, 0.0, None, dW_[0], db_[0], dims[1], oz[0].view, oz[0].ld,
         osp[0].view)
    for i in (1, 2):
        call("mlp_fwd_layer", oz[i - 1].view, oz[i - 1].ld, rows, dims[i], osp[i - 1].view, dga_[i - 1], dbe_[i - 1], EPS, orm[i - 1].view,
             orv[i - 1].view, MOM, ost[i - 1].view, dW_[i], db_[i], dims[i + 1], oz[i].view, oz[i].ld, osp[i].view)
    call("mlp_bn_act", oz[2].view, oz[2].ld, rows, dims[3], osp[2].view, dga_[2], dbe_[2], EPS, orm[2].view, orv[2].view, MOM, ost[2].view, oy.view,
         oy.ld)
    # backward, as _mlp3_backward_fused
    ogp = [Out(dev, nblk, 128, False, torch.float64) for _ in range(3)]
    odw = [Out(dev, nblk, 4096) for _ in range(3)]
    odg, odb = [Out(dev, 1, dims[i + 1]) for i in range(3)], [Out(dev, 1, dims[i + 1]) for i in range(3)]
    odx = [Out(dev, rows, dims[i]) for i in range(3)]
    oW = [Out(dev, 1, dims[i + 1] * dims[i]) for i in range(3)]
    ddy3 = D(dy3)
    call("mlp_bn_bwd_reduce", ddy3, dims[3], oz[2].view, oz[2].ld, rows, dims[3], ost[2].view, ogp[2].view)
    dyv, lddy = ddy3, dims[3]
    for i in (2, 1, 0):
        xin, ldxin = (oz[i - 1].view, oz[i - 1].ld) if i else (dxd, dims[0])
        call("mlp_bwd_layer", dyv, lddy, oz[i].view, oz[i].ld, rows, dims[i + 1], ost[i].view, ogp[i].view, odg[i].view, odb[i].view, xin, ldxin,
             dims[i], ost[i - 1].view if i else None, dW_[i], odx[i].view, odx[i].ld, ogp[i - 1].view if i else None, odw[i].view)
        dyv, lddy = odx[i].view, odx[i].ld
    call("mlp_dw_reduce", rows, 3, odw[0].view, oW[0].view, dims[1], dims[0], odw[1].view, oW[1].view, dims[2], dims[1], odw[2].view, oW[2].view,
         dims[3], dims[2])
    torch.cuda.synchronize()
    k = "chain"
    # forward half, stage by stage
    zc, stc, masks = [o.cpu() for o in oz], [], []
    act, am, cx = x.double(), x.abs().double(), 0
    for i in range(3):
        note = "stage %d of %s" % (i + 1, dims)
        zref = ref_product(act, am, cx, Ws[i], bs[i])
        check(k, "Z", zc[i], *zref, note)
        check_records(k, "out_part", osp[i], rows, *sum_records(zc[i].double(), rows, upper(*zref)), dims[i + 1], note)
        stc.append(check_stats(k, zc[i], gammas[i], betas[i], rm0[i], rv0[i], ost[i], orm[i], orv[i], note))
        mask, val, mag, da, _ = bn_parts(zc[i], stc[i])
        masks.append(mask)
        act, am, cx = mask * val, mask * mag, CACT
        assert oz[i].guards_intact(), note
    check(k, "Y", oy.cpu(), act, masks[2] * U32 * (da + mag), str(dims))
    assert oy.guards_intact()
    # backward half, stage by stage, each fed what the chain handed it
    check_records(k, "g_part", ogp[2], rows, *ref_g_records(dy3, zc[2], stc[2], rows), dims[3], str(dims))
    dyc = dy3
    for i in (2, 1, 0):
        note = "stage %d of %s" % (i + 1, dims)
        rec = ogp[i].cpu().view(nblk, 2, 64)[:, :, :dims[i + 1]]
        ref = ref_bwd(dyc, zc[i], stc[i], rec, zc[i - 1] if i else x, stc[i - 1] if i else None, Ws[i], rows)
        check(k, "dgamma", odg[i].cpu()[0], *ref["dgamma"], note)
        check(k, "dbeta", odb[i].cpu()[0], *ref["dbeta"], note)
        check(k, "dX", odx[i].cpu(), *ref["dX"], note)
        check_dw_part(k, odw[i], ref["dW_part"], rows, dims[i + 1], dims[i], note)
        if i:
            check_records(k, "gprev_part", ogp[i - 1], rows, *gprev_records(odx[i].cpu(), ref["dX"], ref["mask_in"], ref["xhat_in"], rows),
                          dims[i], note)
        want = odw[i].cpu().view(nblk, 64, 64)[:, :dims[i + 1], :dims[i]].double().sum(0).float()
        got = oW[i].cpu()[0].view(dims[i + 1], dims[i])
        assert float(((got - want).abs() / (torch.nextafter(want.abs(), torch.tensor(float("inf"))) - want.abs())).max()) <= 1.0, note
        for o in (odg[i], odb[i], odx[i], oW[i]):
            assert o.guards_intact(), note
        dyc = odx[i].cpu()
    # the references the kernels answered to compose to the block's gradient: fp64 autograd with the same masks
    x64 = x.double().requires_grad_(True)
    P = [[t.double().requires_grad_(True) for t in grp] for grp in (Ws, bs, gammas, betas)]
    M = [m.double() for m in masks]
    cur = x64
    for i in range(3):
        zz = cur @ P[0][i].t() + P[1][i]
        cur = M[i] * ((zz - zz.mean(0)) / torch.sqrt(zz.var(0, unbiased=False) + EPS32) * P[2][i] + P[3][i])
    (cur * dy3.double()).sum().backward()
    with torch.no_grad():
        f = _block_by_references(x.double(), *[[t.detach() for t in grp] for grp in P], M, dy3.double(), rows)
    pairs = [("dx", x64.grad)] + [("dW%d" % i, P[0][i].grad) for i in range(3)] + [("dgamma%d" % i, P[2][i].grad) for i in range(3)] \
        + [("dbeta%d" % i, P[3][i].grad) for i in range(3)]
    for nm, want in pairs:
        assert float((f[nm] - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max())), nm
