"""Plain float64 restatements of the kernels of csrc/bn.hip (train-mode BatchNorm statistics and running-stat updates, the eval fold, the
affine + ReLU pass, the BatchNorm backward, the column sums and the copy / mask / fill helpers) with a-priori fp32 rounding bounds, the
host rules of the file restated (which kernel and tile a shape reaches), and an fp32 emulation of every reduction in the order the source
fixes -- for tests/test_bn_kernels_gpu.py and tests/test_bn_ref_cpu.py.  Every function takes the fp32 values a kernel read (CPU tensors)
and returns (reference, bound) pairs in float64; |out - ref| <= MARGIN * bound elementwise is what the GPU tests assert, and the emulation
(emu_* below) has to stay inside the same bounds.

u = U32 = 2^-24 (one fp32 rounding, relative), U64 = 2^-53.  All bounds are first order in u unless a line says otherwise (MARGIN = 4 is
for what they leave out, as in tests/lstm_ref.py); a sum of n terms in ANY order is known to (n - 1) u sum |terms|, written n u below so
that the rounding of each term's own formation is covered where it has one.  Magnitudes inside a bound come from the float64 reference.

  colstats_kernel, one block b of n_b rows (r0 its first), one column.  shift = x[r0];  d_r = fl(x_r - shift): u |d_r|.
      With  D_b = sum |x_r - shift|,  Q_b = sum (x_r - shift)^2,  S_b = sum (x_r - shift)  (float64, exact to U64):
        S   = TR lanes down the rows, then the serial sum over j  (n_b terms, each rounded once):  e(S) = (n_b + 1) u D_b
        SS  = the same order over d * d  (d known to u |d|: 2 u d^2; the product or its fma: u):    e(SS) = (n_b + 3) u Q_b
        mean_d = fl(S / N):  e(S) / n_b + u |mean_d|,   |mean_d| <= D_b / n_b
        mean_b = fl(shift + mean_d):                     e(mean_b) = (n_b + 2) u D_b / n_b + u |mean_b|
        M2_b   = max(fl(SS - S mean_d), 0)  (S mean_d = S^2 / n_b: 2 |S| e(S) / n_b, the division's and the product's rounding 2 u S^2 / n_b,
                 the subtraction or its fma u M2_b + u S^2 / n_b; the clamp moves the value TOWARDS the true M2_b >= 0):
                                                         e(M2_b) = (n_b + 3) u Q_b + 2 (n_b + 1) u D_b |S_b| / n_b + 3 u S_b^2 / n_b + u M2_b
      These are sums of |x - shift|, not |x|: a column 1000 + 0.01 randn has D_b of order 0.01 n_b.  What is left of |x| is the ONE
      rounding of mean_b to fp32, u |mean_b| -- the record format's, not the summation's.
  bn_finalize_kernel, float64 over the records (n_b, mean_b, M2_b), B = nblk:
        mean = sum n_b mean_b / N:                       e(mean) = sum n_b e(mean_b) / N + (B + 2) U64 sum n_b |mean_b| / N
        M2 = sum [M2_b + n_b (mean_b - mean)^2].  With the TRUE block means this is exactly sum (x - mean)^2; with means off by
        delta_b = e(mean_b) + e(mean) each square moves by  2 |mean_b - mean| delta_b + delta_b^2  (the second-order term is kept: where
        every block mean equals the mean the first-order term vanishes):
                                                         e(M2) = sum e(M2_b) + sum n_b (2 |mean_b - mean| delta_b + delta_b^2) + (B + 4) U64 M2
        var = M2 / N;  invstd = fp32(1 / sqrt(var + eps)) from float64:  |d invstd| <= e(var) / 2 (max(var - e(var), 0) + eps)^1.5  (the
        mean-value theorem with the derivative at the smallest argument; NOT first order) + u invstd
        mean_out = fp32(mean): e(mean) + u |mean|;   a = fl(gamma invstd): |gamma| e(invstd) + u |a| and, from the kernel's OWN stored
        invstd, one product: bits;   b = beta: bits.
        unbiased = M2 / (N - 1), and var where N == 1 (the kernel's rule: `N > 1.0 ? M2 / (N - 1.0) : var`; torch has NaN there), rounded
        to fp32: e(M2) / (N - 1) + u |unbiased|.
        running = fl(1 - mom) * old + mom * new, two products and a sum of which the compiler may fuse one:
            2 u |(1 - mom) old|  (the rounding of 1 - mom and of the product)  + u |mom new| + u |running| + |mom| e(new)
        mom == 0: fl(1 - 0) = 1, 1 * old = old, 0 * new = +-0 for every finite new, old + +-0 = old for every old != 0, fused or not:
        the running statistics keep their bits (a running value of -0.0 would turn into +0.0; the tests use none).  mom == 1:
        fl(1 - 1) = 0, 0 * old = +-0, +-0 + 1 * new = new: running_mean == mean_out.
  finalize alone  the records are inputs, exact: e(mean_b) = e(M2_b) = 0 above; what is left is U64 and the final roundings.
  bn_eval_affine  invstd = 1.0f / sqrtf(fl(rv + eps)): the sum's u enters as u / 2; ASSUMPTION: sqrtf and the division are each within
                  1 ulp = 2 u (the bound HIP documents for sqrtf; the division is correctly rounded as this library is built):
                  e(invstd) = 4.5 u invstd.  a: |gamma| e(invstd) + u |a|, bits from the own invstd; mean_out, b: bits.
  bn_fold_linear  s = fl(gamma / sqrtf(fl(rv + eps))): 4.5 u |s|;  Wf = fl(s W): 5.5 u |s W|;
                  bf = fl(fl(b - rm) s + beta), fused or not: with t = b - rm,  6.5 u |t s| + u |bf|  (u |t|, 4.5 u from s, one product).
  affine_act      v1 = (x1 - m1) a1 + b1: 2 u |(x1 - m1) a1| + u |v1|;  two inputs: e(v1) + e(v2) + u |v1 + v2| (contraction fuses, it
                  does not reassociate);  relu: max(v, 0) moves no value away from max(ref, 0).
  bn_backward     g = dY where mask > 0, else 0 (NaN, +-0 and negatives fail `> 0`; a positive denormal passes);  xh = fl(fl(x - mu) is):
                  2 u |xh|.  Per block (n_b <= RPB rows) s1 = sum g: RPB u sum |g|;  s2 = sum g xh: (RPB + 3) u sum |g xh|;  float64 across
                  the blocks: (B + 1) U64 sum |.|;  dbeta = fp32(s1), dgamma = fp32(s2): + u |s|.
                  c1 = fp32(s1 / rows): e(s1) / rows + u |c1|;  c2 alike.
                  dX = fl(a fl(fl(g - c1) - xh c2)):  |a| [e(c1) + u |g - c1| + |xh| e(c2) + 3 u |xh c2| + u |g - c1 - xh c2|] + u |dX|.
  colsum, short   every addition is float64 (rows U64 sum |x|), one rounding to fp32: u |sum| -- the sum is essentially correctly
                  rounded, whatever cancels.  scale: fl(fp32(sum) scale[c]): bits from an unscaled call; accumulate: fl(old + new):
                  bits from a call without (with BOTH the product may fuse into the sum: e(new) |scale| ... + u |out|, a bound only).
  colsum, long    per block of n_b rows (RPB, or 128 in colsum_partial4_kernel) an fp32 sum: n_b u sum_b |x|;  float64 across the blocks;
                  fp32(sum): u |sum|;  accumulate: u |out|.
  copy2d, copy2d_pair, relu_mask, fill: bits (copy2d with accumulate: the bits of the fp32 sum x + y)."""
import torch

from lstm_ref import U32, MARGIN, ULP, D, cdiv, gen_for, worst_ratio  # noqa: F401  (re-exported: one definition for all families)

U64 = 2.0 ** -53
SQRT_ULP, DIV_ULP = 1.0, 1.0
E_RSQRT = 0.5 * U32 + (SQRT_ULP + DIV_ULP) * ULP            # relative error of 1 / sqrtf(fl(v + eps)), and of gamma / sqrtf(..)
EW_CAP = 2048 * 256                                         # elements one pass of the capped elementwise grid covers


# ---------------------------------------------------------------------------------------------------------------------------------
# host rules of bn.hip, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def rows_per_block(rows):
    r = max(16, (rows + 1023) // 1024)
    return (r + 3) // 4 * 4


def col_tile(C):
    tc = 8
    while tc < C and tc < 64:
        tc <<= 1
    return tc


def nblk(rows):
    return cdiv(rows, rows_per_block(rows))


def ew_blocks(total):
    return min(2048, max(1, cdiv(total, 256)))


def ew_passes(total):
    """How often a thread of the capped grid walks round its loop (2: the grid-stride loop is entered a second time)."""
    return cdiv(total, ew_blocks(total) * 256)


def short_tile(C):
    return 16 if C >= 16 else col_tile(C)


def colsum_path(rows, C, ld, aligned=True):
    """-> (kernel, TC, rows per block, blocks) of mmego_colsum; aligned: X on a 16-byte address."""
    if rows <= 1024:
        return "colsum_small_kernel", short_tile(C), rows, 1
    if rows >= 4096 and C >= 256 and C % 4 == 0 and ld % 4 == 0 and aligned and cdiv(rows, 128) <= nblk(rows):
        return "colsum_partial4_kernel", 16, 128, cdiv(rows, 128)
    return "colsum_partial_kernel", col_tile(C), rows_per_block(rows), nblk(rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# case lists (the GPU file runs them, the CPU file pins what each reaches and runs the emulation over them)
# ---------------------------------------------------------------------------------------------------------------------------------
ROWS = (1, 2, 15, 16, 17, 37, 1024, 1025, 16385)
CS = (1, 3, 8, 27, 45, 64, 65, 130)
CONFIGS = ((True, 0.1, 1e-5), (False, 0.1, 1e-5), (True, 1.0, 1e-3), (True, 0.0, 1e-5))          # running stats given, momentum, eps
STATS_CASES = [(r, c) + CONFIGS[(i + j) % 4] for i, r in enumerate(ROWS) for j, c in enumerate((3, 27, 65, 130))] + \
              [(17, 1) + CONFIGS[0], (37, 8) + CONFIGS[2], (1025, 45) + CONFIGS[3], (16, 64) + CONFIGS[1], (16385, 8) + CONFIGS[2]]
FINALIZE_NBLK = (1, 63, 64, 65, 1023, 1024)
PAIR_CASES = ((37, 8), (1025, 16), (17, 64), (2, 128), (16385, 16))
EVAL_C = (1, 63, 64, 65, 130)
FOLD_CASES = ((1, 1), (3, 7), (64, 64), (130, 33), (2049, 256))
AFFINE_CASES = ((1, 1), (17, 3), (37, 65), (1025, 27), (4033, 130))
BWD_CASES = [(r, c, bool((i + j) & 1)) for i, r in enumerate(ROWS) for j, c in enumerate((3, 27, 65))] + \
            [(37, 130, True), (1025, 8, False), (16385, 45, True), (17, 1, True), (16, 64, False)]
BWD_PAIR_CASES = ((37, 8), (1025, 64), (16385, 128), (1, 64))
CHAIN_CASES = ((37, 27), (1025, 64), (16385, 8))
CHAIN_PAIR = (37, 64)
SHORT_ROWS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1024)
SHORT_CS = (1, 5, 8, 15, 16, 17, 65, 260)
# (rows, C, ld, lead floats in front of X, kernel)
LONG_CASES = ((1025, 5, 7, 0, "colsum_partial_kernel"), (4096, 256, 260, 0, "colsum_partial4_kernel"), (4095, 256, 260, 0, "colsum_partial_kernel"),
              (4096, 252, 256, 0, "colsum_partial_kernel"), (4096, 256, 260, 1, "colsum_partial_kernel"), (4096, 256, 257, 0, "colsum_partial_kernel"),
              (4100, 260, 264, 0, "colsum_partial4_kernel"), (16385, 130, 133, 0, "colsum_partial_kernel"),
              (131200, 256, 260, 0, "colsum_partial_kernel"))
# the last: cdiv(rows, 128) = 1025 > nblk = 994, the one condition of the path choice that only a tensor past 131072 rows x 256 columns
# can fail (134 MB, the smallest there is; everything else in this file stays below 16385 x 130 floats)
LONG_BLOCKS_RULE = (131200, 256)
PAIR_SUM_ROWS, PAIR_SUM_CS = (1, 37, 512, 1024), (16, 64, 256)
COLSUM2_CASES = ((37, 65, 23, 1), (1024, 260, 129, 16), (1, 1, 2, 1))          # rows1, C1, rows2, C2
COPY_CASES = ((1, 1), (37, 45), (300, 128), (4033, 130))
FILL_N = (1, 255, 256, 257, EW_CAP + 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
KINDS = ("randn", "large mean", "constant", "block outlier", "one nonzero", "cancelling")
CANCEL, CONST = 5, 0.1


def columns(rows, C, key, first=0, block=None):
    """-> (X [rows][C] fp32, kinds [C]): column c is of kind (first + c) % 6.  block: the rows per block whose first row is the outlier
    (default: rows_per_block(rows))."""
    g = gen_for(rows, C, key, 41)
    X = torch.randn(rows, C, generator=g)
    kinds = (torch.arange(C) + first) % 6
    r = torch.arange(rows)
    blk = block or rows_per_block(rows)
    for c in range(C):
        k = int(kinds[c])
        if k == 1:
            X[:, c] = 1000.0 + 0.01 * X[:, c]
        elif k == 2:
            X[:, c] = CONST
        elif k == 3:
            X[r % blk == 0, c] = 1e4
        elif k == 4:
            X[:, c] = 0.0
            X[(7 * c + 3) % rows, c] = 2.5
        elif k == 5:
            X[:, c] = torch.where(r % 2 == 0, 1e4, -1e4) + X[:, c]
    return X, kinds


def bn_params(C, key):
    """gamma (either sign), beta, running mean, running variance (none of them zero)."""
    g = gen_for(C, key, 43)
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    return gamma, torch.randn(C, generator=g) * 0.3 + 0.05, torch.randn(C, generator=g) * 0.4 + 0.01, torch.rand(C, generator=g) + 0.5


def stats_inputs(case):
    """A STATS_CASES entry -> X, kinds, the arguments behind X of train_stats / emu_train_stats."""
    rows, C, running, mom, eps = case
    X, kinds = columns(rows, C, 11)
    g, b, rm, rv = bn_params(C, 11)
    return X, kinds, (g, b, rm if running else None, rv if running else None, mom, eps)


def colsum_inputs(rows, C, key=0):
    """X [rows][C] of every kind of column, the cancelling one first; old values of out; scale."""
    X, _ = columns(rows, C, 17 + key, first=CANCEL, block=16)
    g = gen_for(rows, C, 18)
    return X, torch.randn(C, generator=g), torch.randn(C, generator=g)


def given_state(C, key):
    """mean, invstd, a that are NOT the batch's own (the backward is a formula of the state it is handed)."""
    g = gen_for(C, key, 47)
    return torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5, (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)


def mask_values(rows, C, key):
    """A ReLU mask of every kind: positives, negatives, +0, -0, denormals of both signs, NaN."""
    g = gen_for(rows, C, key, 53)
    M = torch.randn(rows, C, generator=g)
    sel = torch.randint(0, 12, (rows, C), generator=g)
    for v, val in ((0, 0.0), (1, -0.0), (2, 1e-40), (3, -1e-40), (4, float("nan"))):
        M[sel == v] = val
    return M


def passes(mask, like):
    return torch.ones_like(like, dtype=torch.bool) if mask is None else mask > 0


def hand_records(nb, C, key):
    """Records (n_b, mean_b, M2_b) [nb][C] as the GCN front kernel hands them over: unequal n_b, the last block a single row with
    M2 = 0, block means far apart (steps of 50 against a spread of 1)."""
    g = gen_for(nb, C, key, 59)
    n = torch.randint(1, 40, (nb, 1), generator=g).float().expand(nb, C).clone()
    n[-1] = 1.0
    m = torch.randn(nb, C, generator=g) + 50.0 * torch.randint(-3, 4, (nb, C), generator=g).float()
    q = torch.rand(nb, C, generator=g) * n
    q[n == 1] = 0.0
    return n, m, q


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references with bounds: statistics
# ---------------------------------------------------------------------------------------------------------------------------------
def blocked(T, rpb, fill=0.0):
    """[rows][C] -> ([B][rpb][C] padded with `fill`, valid [B][rpb][1])"""
    rows, C = T.shape
    B = cdiv(rows, rpb)
    P = torch.full((B * rpb, C), fill, dtype=T.dtype)
    P[:rows] = T
    valid = (torch.arange(B * rpb) < rows).view(B, rpb, 1)
    return P.view(B, rpb, C), valid


def record_bounds(X):
    """-> n [B][1], mean_b [B][C], e(mean_b), e(M2_b) of colstats_kernel's records, float64."""
    rows = X.shape[0]
    P, valid = blocked(D(X), rows_per_block(rows))
    d = (P - P[:, :1]) * valid
    n = valid.sum(1).double()
    S, Dabs, Q = d.sum(1), d.abs().sum(1), (d * d).sum(1)
    mean_b = P[:, 0] + S / n
    M2_b = (Q - S * S / n).clamp_min(0.0)
    e_m = (n + 2) * U32 * Dabs / n + U32 * mean_b.abs()
    e_q = (n + 3) * U32 * Q + 2 * (n + 1) * U32 * Dabs * S.abs() / n + 3 * U32 * S * S / n + U32 * M2_b
    return n, mean_b, e_m, e_q


def pooled_bounds(n, m, e_m, e_q, mean, M2):
    """e(mean), e(M2) of bn_finalize_kernel's pooling of records known to e_m, e_q (mean, M2: the float64 reference)."""
    B, N = n.shape[0], n.sum(0)
    e_mean = (n * e_m).sum(0) / N + (B + 2) * U64 * (n * m.abs()).sum(0) / N
    delta = e_m + e_mean
    e_M2 = e_q.sum(0) + (n * (2 * (m - mean).abs() * delta + delta * delta)).sum(0) + (B + 4) * U64 * M2
    return e_mean, e_M2


def state_of(N, mean, e_mean, M2, e_M2, gamma, beta, rm, rv, mom, eps):
    """Everything bn_finalize_kernel writes, from pooled statistics known to e_mean, e_M2: {name: (ref, bound)}.  mom, eps: the fp32
    values the kernel receives."""
    mom, eps = float(torch.tensor(mom, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32))
    var, e_var = M2 / N, e_M2 / N
    invstd = 1.0 / torch.sqrt(var + eps)
    e_inv = 0.5 * e_var * ((var - e_var).clamp_min(0.0) + eps) ** -1.5 + U32 * invstd
    a = D(gamma) * invstd
    out = {"mean": (mean, e_mean + U32 * mean.abs()), "invstd": (invstd, e_inv), "a": (a, D(gamma).abs() * e_inv + U32 * a.abs()),
           "b": (D(beta), torch.zeros_like(mean))}
    if rm is not None:
        unb = M2 / (N - 1.0) if N > 1 else var          # N == 1: the biased value, the kernel's rule
        e_unb = e_M2 / max(N - 1.0, 1.0) + U32 * unb.abs()
        for name, old, new, e_new in (("running_mean", D(rm), mean, out["mean"][1]), ("running_var", D(rv), unb, e_unb)):
            ref = (1.0 - mom) * old + mom * new
            out[name] = (ref, 2 * U32 * ((1.0 - mom) * old).abs() + U32 * (mom * new).abs() + U32 * ref.abs() + abs(mom) * e_new)
    return out


def train_stats(X, gamma, beta, rm, rv, mom, eps):
    """mmego_bn_train_stats of X [rows][C]: two-pass float64 statistics, the bounds of colstats_kernel + bn_finalize_kernel."""
    Xd = D(X)
    N = float(X.shape[0])
    mean = Xd.mean(0)
    M2 = ((Xd - mean) ** 2).sum(0)
    n, m, e_m, e_q = record_bounds(X)
    e_mean, e_M2 = pooled_bounds(n, m, e_m, e_q, mean, M2)
    return state_of(N, mean, e_mean, M2, e_M2, gamma, beta, rm, rv, mom, eps)


def pooled(n, m, q):
    """Float64 pooled statistics of records: N, mean, M2."""
    n, m, q = D(n), D(m), D(q)
    N = n.sum(0)
    mean = (n * m).sum(0) / N
    return N, mean, (q + n * (m - mean) ** 2).sum(0)


def finalize(n, m, q, gamma, beta, rm, rv, mom, eps):
    """mmego_bn_finalize of exact records [B][C]."""
    N, mean, M2 = pooled(n, m, q)
    zero = torch.zeros_like(D(m))
    e_mean, e_M2 = pooled_bounds(D(n), D(m), zero, zero, mean, M2)
    assert bool((N == N[0]).all())
    return state_of(float(N[0]), mean, e_mean, M2, e_M2, gamma, beta, rm, rv, mom, eps)


def eval_affine(gamma, beta, rm, rv, eps):
    eps = float(torch.tensor(eps, dtype=torch.float32))
    invstd = 1.0 / torch.sqrt(D(rv) + eps)
    e_inv = E_RSQRT * invstd
    a = D(gamma) * invstd
    return {"mean": (D(rm), torch.zeros_like(a)), "invstd": (invstd, e_inv), "a": (a, D(gamma).abs() * e_inv + U32 * a.abs()),
            "b": (D(beta), torch.zeros_like(a))}


def fold_linear(W, b, gamma, beta, rm, rv, eps):
    """-> {"Wf" [N][K], "bf" [N]}"""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    s = D(gamma) / torch.sqrt(D(rv) + eps)
    Wf = s[:, None] * D(W)
    t = (0.0 if b is None else D(b)) - D(rm)
    bf = t * s + D(beta)
    return {"Wf": (Wf, (E_RSQRT + U32) * Wf.abs()), "bf": (bf, (E_RSQRT + 2 * U32) * (t * s).abs() + U32 * bf.abs())}


def affine_pre(X1, m1, a1, b1, X2=None, m2=None, a2=None, b2=None):
    """The pre-activation of mmego_affine_act and its bound."""
    p1 = (D(X1) - D(m1)) * D(a1)
    v = p1 + D(b1)
    e = 2 * U32 * p1.abs() + U32 * v.abs()
    if X2 is not None:
        p2 = (D(X2) - D(m2)) * D(a2)
        v2 = p2 + D(b2)
        e = e + 2 * U32 * p2.abs() + U32 * v2.abs() + U32 * (v + v2).abs()
        v = v + v2
    return v, e


def affine_act(relu, *args):
    v, e = affine_pre(*args)
    return (v.clamp_min(0.0) if relu else v), e


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references with bounds: backward
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_backward(dY, mask, X, mean, invstd, a, e_state=None):
    """-> {"dgamma", "dbeta" [C], "dX" [rows][C]} of mmego_bn_backward: a formula of the GIVEN mean / invstd / a.
    e_state = (e(mean), e(invstd), e(a)) (the chain tests): mean, invstd and a are then the float64 statistics, and the kernel ran on
    fp32 ones known to these bounds.  First order: xh moves by  e(xh) = invstd e(mean) + |x - mean| e(invstd),  s2 by  sum |g| e(xh),
    dX by  |a| |c2| e(xh) + |g - c1 - xh c2| e(a)  and by what c2 moved."""
    rows = X.shape[0]
    rpb, B = rows_per_block(rows), nblk(rows)
    g = torch.where(passes(mask, dY), D(dY), torch.zeros((), dtype=torch.float64))
    xh = (D(X) - D(mean)) * D(invstd)
    s1, s2 = g.sum(0), (g * xh).sum(0)
    A1, A2 = g.abs().sum(0), (g * xh).abs().sum(0)
    e1 = (rpb * U32 + (B + 1) * U64) * A1
    e2 = ((rpb + 3) * U32 + (B + 1) * U64) * A2
    e_xh = e_a = 0.0
    if e_state is not None:
        e_xh = D(invstd) * e_state[0] + (D(X) - D(mean)).abs() * e_state[1]
        e2, e_a = e2 + (g.abs() * e_xh).sum(0), e_state[2]
    c1, c2 = s1 / rows, s2 / rows
    e_c1, e_c2 = e1 / rows + U32 * c1.abs(), e2 / rows + U32 * c2.abs()
    t = g - c1 - xh * c2
    dX = D(a) * t
    e_dX = D(a).abs() * (e_c1 + U32 * (g - c1).abs() + xh.abs() * e_c2 + c2.abs() * e_xh + 3 * U32 * (xh * c2).abs() + U32 * t.abs()) \
        + t.abs() * e_a + U32 * dX.abs()
    return {"dbeta": (s1, e1 + U32 * s1.abs()), "dgamma": (s2, e2 + U32 * s2.abs()), "dX": (dX, e_dX)}


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references with bounds: column sums
# ---------------------------------------------------------------------------------------------------------------------------------
def colsum(X, path, old=None, scale=None):
    """mmego_colsum through `path` (colsum_path's tuple): out = [old +] sum [* scale]."""
    kernel, _, rpb, B = path
    Xd = D(X)
    s, A = Xd.sum(0), Xd.abs().sum(0)
    if kernel == "colsum_small_kernel":
        e = X.shape[0] * U64 * A + U32 * s.abs()
    else:
        e = (rpb * U32 + (B + 1) * U64) * A + U32 * s.abs()
    if scale is not None:
        s, e = s * D(scale), e * D(scale).abs() + U32 * (s * D(scale)).abs()
    if old is not None:
        s = s + D(old)
        e = e + U32 * s.abs()
    return s, e


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulation, in the order the source fixes.  (fp32 torch on the CPU rounds every operation once: no contraction.)
# ---------------------------------------------------------------------------------------------------------------------------------
def emu_block_sums(T, rpb, TR, drop_last=False):
    """colstats_kernel's / bn_bwd_reduce_kernel's / colsum_partial*_kernel's sum of one block's rows of T [rows][C] (fp32 or float64): TR
    lanes down the rows (lane ry takes rows r0 + ry, r0 + ry + TR, ..), then the serial sum over the lanes j.  -> [B][C].  Rows behind
    the last add an exact 0."""
    P, _ = blocked(T, rpb)
    B, _, C = P.shape
    K = cdiv(rpb, TR)
    L = torch.zeros(B, K * TR, C, dtype=T.dtype)
    L[:, :rpb] = P
    L = L.view(B, K, TR, C)
    s = torch.zeros(B, TR, C, dtype=T.dtype)
    for k in range(K):
        s = s + L[:, k]
    a = torch.zeros(B, C, dtype=T.dtype)
    for j in range(TR):
        a = a + s[:, j]
    if drop_last and T.shape[0] % rpb:
        a = a[:-1]
    return a


def emu_wave(V, B, leak=False):
    """The finalize kernels' float64 sum of V [B][C] (B <= 1024): lane l holds records l + 64 u, u = 0..15 -- a record past B is loaded
    from the clamped address 0 and then zeroed (leak: not zeroed) -- sums its 16, then the xor butterfly 32, 16, .., 1."""
    k = torch.arange(1024)
    ok = k < B
    Q = D(V)[torch.where(ok, k, torch.zeros_like(k))]
    if not leak:
        Q = Q * ok.view(-1, 1)
    Q = Q.view(16, 64, -1)
    s = torch.zeros_like(Q[0])
    for u in range(16):
        s = s + Q[u]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[lane ^ o]
    return s[0]


def f32(x):
    return torch.as_tensor(x, dtype=torch.float32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def emu_records(X, TC, mutant=None):
    """colstats_kernel: records n, mean_b, M2_b [B][C] in fp32."""
    rows = X.shape[0]
    rpb, TR = rows_per_block(rows), 256 // TC
    P, valid = blocked(X, rpb)
    shift = torch.zeros_like(P[:, :1]) if mutant == "no shift" else P[:, :1]
    d = ((P - shift) * valid).reshape(-1, X.shape[1])[:rows]
    drop = mutant == "drop last block"
    S, SS = emu_block_sums(d, rpb, TR, drop), emu_block_sums(d * d, rpb, TR, drop)
    n = valid.sum(1).float()[:S.shape[0]].expand_as(S)
    mean_d = S / n
    return n, shift[:S.shape[0], 0] + mean_d, (SS - S * mean_d).clamp_min(0.0)


def emu_finalize(n, m, q, gamma, beta, rm, rv, mom, eps, mutant=None):
    """bn_finalize_kernel on fp32 records [B][C] -> {name: fp32 [C]}"""
    B = n.shape[0]
    leak = mutant == "lanes not zeroed"
    n, m, q = D(n), D(m), D(q)
    N, S = emu_wave(n, B, leak), emu_wave(n * m, B, leak)
    mean = S / N
    dm = m - mean
    M2 = emu_wave(q + n * dm * dm, B, leak)
    var = M2 / N
    mom, eps = f32(mom), f32(eps)
    invstd = (1.0 / torch.sqrt(var + eps.double())).float()
    out = {"mean": mean.float(), "invstd": invstd, "a": gamma * invstd, "b": beta.clone()}
    if rm is not None:
        unb = torch.where(N > 1.0, M2 / (N - 1.0), var)
        if mutant == "biased running var":
            unb = var
        keep, take = (mom, f32(1.0) - mom) if mutant == "momentum on the old value" else (f32(1.0) - mom, mom)
        out["running_mean"] = keep * rm + take * mean.float()
        out["running_var"] = keep * rv + take * unb.float()
    return out


def emu_train_stats(X, gamma, beta, rm, rv, mom, eps, mutant=None):
    return emu_finalize(*emu_records(X, col_tile(X.shape[1]), mutant), gamma, beta, rm, rv, mom, eps, mutant)


def emu_bn_backward(dY, mask, X, mean, invstd, a, mutant=None):
    """bn_bwd_reduce_kernel, bn_bwd_finalize_kernel, bn_bwd_apply_kernel -> dgamma, dbeta, dX (fp32)."""
    rows, C = X.shape
    rpb, TR = rows_per_block(rows), 256 // col_tile(C)
    ok = passes(mask, dY) if mutant != "mask >= 0" else (mask >= 0 if mask is not None else passes(None, dY))
    g = torch.where(ok, dY, torch.zeros(()))
    xh = (X - mean) * invstd
    s1 = emu_wave(emu_block_sums(g, rpb, TR), nblk(rows))
    s2 = emu_wave(emu_block_sums(g * xh, rpb, TR), nblk(rows))
    div = float(rows - 1) if mutant == "rows - 1" else float(rows)
    c1, c2 = (s1 / div).float(), (s2 / div).float()
    t = g - c1
    if mutant != "no xhat c2":
        t = t - xh * c2
    return s2.float(), s1.float(), a * t


def emu_colsum_small(X, TC, old=None, scale=None, seg=0, mutant=None):
    """colsum_small_kernel over X [rows][C] -> (outA, out2A, outB, out2B) in fp32 (B: the columns [seg, C), empty when seg == 0); old:
    (oldA, oldB) under accumulate.  Lane ry adds its rows four at a time, (v0 + v1) + (v2 + v3) in float64, while four remain, then one
    at a time; the lanes are summed serially; one rounding to fp32."""
    rows, C = X.shape
    TR = 256 // TC
    K = cdiv(cdiv(rows, TR), 4) * 4
    L = torch.zeros(K * TR, C, dtype=torch.float64)
    L[:rows] = D(X)
    L = L.view(K, TR, C)
    left = ((rows - torch.arange(TR) + TR - 1) // TR).clamp_min(0).view(TR, 1)          # rows of lane ry
    s = torch.zeros(TR, C, dtype=torch.float64)
    for k in range(0, K, 4):
        v0, v1, v2, v3 = L[k], L[k + 1], L[k + 2], L[k + 3]
        s = torch.where(k + 3 < left, s + ((v0 + v1) + (v2 + v3)), (((s + v0) + v1) + v2) + v3)
    a = torch.zeros(C, dtype=torch.float64)
    for j in range(TR):
        a = a + s[j]
    af = a.float()
    c = torch.arange(C)
    split = seg + 16 if mutant == "seg off by one tile" else seg
    inB = (c >= split) if seg > 0 else torch.zeros(C, dtype=torch.bool)
    cc = torch.where(inB, c - seg, c)
    if scale is not None:
        af = af * (scale[cc] if mutant == "scale[cc]" else scale)
    A, A2 = torch.full((C + 16,), float("nan")), torch.full((C + 16,), float("nan"))
    Bv, B2 = torch.full((C + 16,), float("nan")), torch.full((C + 16,), float("nan"))
    oldv = torch.zeros(C)
    if old is not None:
        both = torch.cat((old[0], torch.zeros(C + 16 - old[0].numel()))), torch.cat((old[1], torch.zeros(C + 16 - old[1].numel())))
        oldv = torch.where(inB, both[1][cc], both[0][cc])
    v = oldv + af if old is not None else af
    v2 = af if mutant == "out2 before accumulation" else v
    A[cc[~inB]], A2[cc[~inB]] = v[~inB], v2[~inB]
    Bv[cc[inB]], B2[cc[inB]] = v[inB], v2[inB]
    nA = seg if seg > 0 else C
    return A[:nA], A2[:nA], Bv[:C - nA], B2[:C - nA]


def emu_colsum(X, path, old=None, scale=None, mutant=None):
    """mmego_colsum through `path` -> (out, out2) in fp32."""
    kernel, TC, rpb, B = path
    if kernel == "colsum_small_kernel":
        return emu_colsum_small(X, TC, None if old is None else (old, old[:0]), scale, 0, mutant)[:2]
    TR = 16 if kernel == "colsum_partial4_kernel" else 256 // TC
    part = emu_block_sums(X, rpb, TR, mutant == "drop last block")
    s = emu_wave(part, part.shape[0], mutant == "lanes not zeroed").float()
    v = old + s if old is not None else s
    return v, (s if mutant == "out2 before accumulation" else v)
