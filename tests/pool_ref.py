"""Plain float64 restatements of the pooling and attention kernels of csrc/pool.hip (attention pooling forward and backward, the group
sums and broadcasts, cross attention forward, pooled forward and backward) with a-priori fp32 rounding bounds, for
tests/test_pool_kernels_gpu.py and tests/test_pool_ref_cpu.py.  Every function takes the fp32 values a kernel read (CPU tensors) and
returns (reference, bound) pairs in float64; |out - ref| <= MARGIN * bound elementwise is what the GPU tests assert, and an fp32
emulation of the same expressions (emu_* below) has to stay inside the bounds WITHOUT the margin (test_pool_ref_cpu.py).

u = 2^-24 (one fp32 rounding, relative).  Bound forms, all first order (MARGIN = 4 is for what they leave out, as in tests/lstm_ref.py):

  dot product      of n terms, in any order, fused or not:  (n + 1) u sum |terms|  [+ sum e(a_k) |b_k| for an operand known to e(a)].
                   An addend in front of or behind the sum (the score's bias, the query projection's) counts as one more term.
  softmax          a_p = e_p / sum_q e_q,  e_p = expf(s_p - m).  The kernel's m is the largest of its OWN fp32 scores; any common shift
                   cancels in the quotient, so m carries no error and the argument's is  e(d_p) = e(s_p) + u |d_p|  (the subtraction).
                   ASSUMPTION: expf (the libm form, OCML's) is accurate to EXPF_ULP = 3 ulp, the bound OpenCL's full profile sets for
                   exp and OCML is built to; no document in this tree gives a tighter one.  An absolute error of the argument is a
                   relative error of exp:
                     rel(e_p) = e(d_p) + 3 ulp
                     rel(sum) = sum_q a_q rel(e_q) + n u            (n additions of non-negative terms, any order)
                     rel(a_p) = rel(e_p) + rel(sum) + 2 u           (1.0f / sum is a correctly rounded division; one product)
                   Every bound carries the absolute floor TINY = 2^-126: below it expf returns a denormal or 0 (a score behind the
                   largest by more than 87 has the weight exactly 0 in fp32 and of order 1e-38 or less in float64).
  weighted sum     vec_c = sum_p x_pc a_p:  (P + 1) u sum |x a| + sum |x_pc| e(a_p)          (cross attention: 16 keys, one masked)
  pooling backward da_p = x_p . dvec: (C + 1) u sum |x dvec|;  dot = sum a_p da_p: sum a_p e(da_p) + (P + 1) u sum |a da|;
                   ds_p = a_p (da_p - dot): |a_p| (e(da_p) + e(dot)) + 2 u |ds_p|  -- ABSOLUTE where da_p - dot cancels (a one-hot row);
                   pdb = sum ds: sum e(ds) + P u sum |ds|;  pdw_c = sum ds_p x_pc: (P + 1) u sum |ds x| + sum e(ds_p) |x_pc|;
                   dX_pc = a_p dvec_c + ds_p w_c (one product rounded, one fma): 2 u (|a dvec| + |ds w|) + e(ds_p) |w_c|.
                   attn is an INPUT of the backward (the fp32 values handed to the kernel), exact.
  cross attention  S = scale Q K^T: (64 + 2) u scale sum |q k| (the product with scale is one more rounding); softmax as above over 15
                   keys (n = 16: the matrix-pipe kernel adds the masked 16th slot's zero); O = P V: 17 u sum |p v| + sum e(p) |v|;
                   pooled: osum = sum over the 64 queries: sum e(O) + 64 u sum |O|; with the query projection inside, Q = X Wq^T + bq
                   is known to (64 + 2) u (sum |x w| + |bq|) and S gains scale sum e(q_c) |k_c|.
                   backward (P an input): dP = dO V^T: 65 u sum |dO v|; dot = sum_j P_j dP_j: sum P e(dP) + 16 u sum |P dP|;
                   dS = P (dP - dot) scale: |P| scale (e(dP) + e(dot)) + 3 u |dS|; dQ = dS K: 16 u sum |dS k| + sum e(dS) |k|;
                   dV = P^T dO: 65 u sum |p dO|; dK = dS^T Q: 65 u sum |dS q| + sum e(dS) |q|.
  group sum        scale sum_p x_p in row order: P u |scale| sum |x| (P - 1 additions and the product); the GPU test also asks for
                   the bits of the fp32 row-order sum.  broadcast: u |scale dY| (+ u |dX + scale dY| when it accumulates).
Magnitudes inside a bound always come from the float64 reference."""
import numpy as np
import torch

from lstm_ref import U32, MARGIN, TINY, ULP, D, cdiv, gen_for, worst_ratio  # noqa: F401  (re-exported: one definition for all families)

EXPF_ULP = 3.0
NQ, NK, DH = 64, 15, 64
BWD_STATIC_LDS = 8224        # attn_pool_bwd_lds_kernel's group segment: dvs[1024], ps[1024], red[8]
FWD_STATIC_LDS = 8224        # attn_pool_fwd_lds_kernel's: wsh[1024], part[1024], red[8]


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references with bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def softmax_b(s, e_s, n):
    """softmax over the last axis of scores known to e_s -> (a, e(a)); n: the additions of the normaliser."""
    d = s - s.max(-1, keepdim=True).values
    E = torch.exp(d)
    a = E / E.sum(-1, keepdim=True)
    rel = e_s + U32 * d.abs() + EXPF_ULP * ULP
    rel_a = rel + (a * rel).sum(-1, keepdim=True) + (n + 2) * U32
    return a, a * rel_a + TINY


def attn_pool_fwd(X, w, b):
    """X [G][P][C], w [C], b (a float or None) -> {"s", "attn" [G][P], "vec" [G][C]: (ref, bound)}"""
    X, w, b = D(X), D(w), 0.0 if b is None else float(b)
    P, C = X.shape[1], X.shape[2]
    t = X * w
    s = t.sum(-1) + b
    e_s = (C + 2) * U32 * (t.abs().sum(-1) + abs(b))
    a, e_a = softmax_b(s, e_s, P)
    vec = torch.einsum("gp,gpc->gc", a, X)
    e_vec = (P + 1) * U32 * torch.einsum("gp,gpc->gc", a, X.abs()) + torch.einsum("gp,gpc->gc", e_a, X.abs())
    return {"s": (s, e_s), "attn": (a, e_a), "vec": (vec, e_vec)}


def attn_pool_bwd(X, w, attn, dvec):
    """X [G][P][C], w [C], attn [G][P] (as given), dvec [G][C] -> {"dX" [G][P][C], "pdw" [G][C], "pdb" [G]: (ref, bound)}"""
    X, w, a, dv = D(X), D(w), D(attn), D(dvec)
    P, C = X.shape[1], X.shape[2]
    t = X * dv[:, None, :]
    da, e_da = t.sum(-1), (C + 1) * U32 * t.abs().sum(-1)
    ad = a * da
    dot = ad.sum(-1, keepdim=True)
    e_dot = (a.abs() * e_da).sum(-1, keepdim=True) + (P + 1) * U32 * ad.abs().sum(-1, keepdim=True)
    ds = a * (da - dot)
    e_ds = a.abs() * (e_da + e_dot) + 2 * U32 * ds.abs()
    pdb, e_pdb = ds.sum(-1), e_ds.sum(-1) + P * U32 * ds.abs().sum(-1)
    t1, t2 = a[:, :, None] * dv[:, None, :], ds[:, :, None] * w
    dX, e_dX = t1 + t2, 2 * U32 * (t1.abs() + t2.abs()) + e_ds[:, :, None] * w.abs()
    pdw = torch.einsum("gp,gpc->gc", ds, X)
    e_pdw = (P + 1) * U32 * torch.einsum("gp,gpc->gc", ds.abs(), X.abs()) + torch.einsum("gp,gpc->gc", e_ds, X.abs())
    return {"dX": (dX, e_dX), "pdw": (pdw, e_pdw), "pdb": (pdb, e_pdb)}


def query_proj(X, Wq, bq):
    """X [F][64][64] point features -> Q = X Wq^T + bq and its bound."""
    X, Wq, bq = D(X), D(Wq), D(bq)
    return X @ Wq.t() + bq, (DH + 2) * U32 * (X.abs() @ Wq.abs().t() + bq.abs())


def cross_fwd(Q, K, V, scale, e_Q=None):
    """Q [F][64][64] (float64 with e_Q, or the fp32 operand), K, V [F][15][64] -> {"P" [F][64][15], "O" [F][64][64], "osum" [F][64]}"""
    Q, K, V = D(Q), D(K), D(V)
    S = scale * (Q @ K.transpose(1, 2))
    e_S = (DH + 2) * U32 * scale * (Q.abs() @ K.abs().transpose(1, 2))
    if e_Q is not None:
        e_S = e_S + scale * (e_Q @ K.abs().transpose(1, 2))
    Pm, e_P = softmax_b(S, e_S, NK + 1)
    O = Pm @ V
    e_O = (NK + 2) * U32 * (Pm @ V.abs()) + e_P @ V.abs()
    return {"S": (S, e_S), "P": (Pm, e_P), "O": (O, e_O), "osum": (O.sum(1), e_O.sum(1) + NQ * U32 * O.abs().sum(1))}


def cross_bwd(Q, K, V, Pm, dO, scale):
    """P as given -> {"dQ" [F][64][64], "dK", "dV" [F][15][64]: (ref, bound)}"""
    Q, K, V, Pm, dO = D(Q), D(K), D(V), D(Pm), D(dO)
    dP, e_dP = dO @ V.transpose(1, 2), (DH + 1) * U32 * (dO.abs() @ V.abs().transpose(1, 2))
    pd = Pm * dP
    dot = pd.sum(-1, keepdim=True)
    e_dot = (Pm.abs() * e_dP).sum(-1, keepdim=True) + (NK + 1) * U32 * pd.abs().sum(-1, keepdim=True)
    dS = Pm * (dP - dot) * scale
    e_dS = Pm.abs() * abs(scale) * (e_dP + e_dot) + 3 * U32 * dS.abs()
    dQ, e_dQ = dS @ K, (NK + 1) * U32 * (dS.abs() @ K.abs()) + e_dS @ K.abs()
    dV, e_dV = Pm.transpose(1, 2) @ dO, (NQ + 1) * U32 * (Pm.abs().transpose(1, 2) @ dO.abs())
    dK = dS.transpose(1, 2) @ Q
    e_dK = (NQ + 1) * U32 * (dS.abs().transpose(1, 2) @ Q.abs()) + e_dS.transpose(1, 2) @ Q.abs()
    return {"dS": (dS, e_dS), "dQ": (dQ, e_dQ), "dK": (dK, e_dK), "dV": (dV, e_dV)}


def group_sum(X, scale):
    """X [G][P][C] -> scale * sum over the P rows"""
    X = D(X)
    return scale * X.sum(1), X.shape[1] * U32 * abs(scale) * X.abs().sum(1)


def group_bcast(dY, P, scale, dX0=None):
    """dY [G][C] -> dX [G][P][C] = scale dY (+ dX0)"""
    v = (scale * D(dY))[:, None, :].expand(-1, P, -1)
    if dX0 is None:
        return v.clone(), U32 * v.abs()
    r = D(dX0) + v
    return r, U32 * (v.abs() + r.abs())


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations of the kernels' forms, in their summation orders where the source fixes one
# ---------------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32 fma (what -ffp-contract=on makes of `acc += a * b`), exact for normal results: the product is exact in float64; the sum is
    rounded to 53 bits with its error kept (TwoSum), and where that lands exactly on an fp32 midpoint while the true sum does not, it is
    moved one float64 step towards the true sum before the rounding to 24 bits (no double rounding)."""
    p, c = a.double() * b.double(), c.double()
    s = p + c
    tie = (s.contiguous().view(torch.int64) & ((1 << 29) - 1)) == (1 << 28)
    if bool(tie.any()):
        p, c = torch.broadcast_tensors(p, c)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = tie & (err != 0) & torch.isfinite(s)
        s = torch.where(fix, torch.nextafter(s, torch.where(err > 0, float("inf"), float("-inf")).double()), s)
    return s.float()


def wave_sum32(v):
    """wave_sum of common.h over the last axis (64 lanes): v += shfl_xor(v, o) for o = 32, 16, .., 1"""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v


def _pad(t, dim, mult):
    n = t.shape[dim]
    m = cdiv(n, mult) * mult
    if m == n:
        return t
    shape = list(t.shape)
    shape[dim] = m - n
    return torch.cat((t, t.new_zeros(shape)), dim)


def emu_dots_wave(X, W):
    """X [G][P][C] . W [G or 1][C] by one wave per row: lane l takes c = l, l + 64, .. in turn (fma), then wave_sum."""
    G, P, _ = X.shape
    Xp, Wp = _pad(X, 2, 64), _pad(W, 1, 64)
    n = Xp.shape[2] // 64
    Xp, Wp = Xp.view(G, P, n, 64), Wp.view(-1, 1, n, 64)
    s = torch.zeros(G, P, 64)
    for i in range(n):
        s = fma32(Xp[:, :, i], Wp[:, :, i], s)
    return wave_sum32(s)[..., 0]


def emu_dots_tpp(X, W, TPP):
    """The LDS kernels' wide form: TPP threads per row, thread pt over channels pt len .. (pt + 1) len - 1 entered at offset p
    (c = c0 + (i + p) % len), partials added in the order pt = 0, 1, .."""
    G, P, C = X.shape
    ln = C // TPP
    idx = (torch.arange(TPP).view(1, TPP, 1) * ln + (torch.arange(ln).view(1, 1, ln) + torch.arange(P).view(P, 1, 1)) % ln)   # [P][TPP][len]
    Xg = torch.gather(X, 2, idx.view(1, P, C).expand(G, -1, -1)).view(G, P, TPP, ln)
    Wg = W[:, idx.view(-1)].view(-1, P, TPP, ln)
    s = torch.zeros(G, P, TPP)
    for i in range(ln):
        s = fma32(Xg[..., i], Wg[..., i], s)
    out = s[..., 0]
    for pt in range(1, TPP):
        out = out + s[..., pt]
    return out


def emu_dots_reg(X, w):
    """attn_pool_fwd_reg_kernel: thread t holds channels 4t .. 4t + 3, (x0 w0 + x1 w1) + (x2 w2 + x3 w3), wave_sum in each of the four
    waves, (part0 + part1) + (part2 + part3)."""
    G, P, _ = X.shape
    Xp, wp = _pad(X, 2, 1024).view(G, P, 4, 64, 4), _pad(w.view(1, -1), 1, 1024).view(1, 1, 4, 64, 4)
    s = fma32(Xp[..., 0], wp[..., 0], Xp[..., 1] * wp[..., 1]) + fma32(Xp[..., 2], wp[..., 2], Xp[..., 3] * wp[..., 3])
    part = wave_sum32(s)[..., 0]                          # [G][P][4]
    return (part[..., 0] + part[..., 1]) + (part[..., 2] + part[..., 3])


def emu_block_sum(v, prod=None):
    """sum over the last axis by a 256-thread workgroup: thread t takes p = t, t + 256, .. in turn (fma with `prod` given: v * prod),
    wave_sum, the four waves' results added in order from 0."""
    G = v.shape[0]
    vp = _pad(v, 1, 256).view(G, -1, 4, 64)
    pp = None if prod is None else _pad(prod, 1, 256).view(G, -1, 4, 64)
    s = torch.zeros(G, 4, 64)
    for i in range(vp.shape[1]):
        s = s + vp[:, i] if pp is None else fma32(vp[:, i], pp[:, i], s)
    r = wave_sum32(s)[..., 0]
    out = torch.zeros(G)
    for wv in range(4):
        out = out + r[:, wv]
    return out


def emu_colsum(X, a, PG=1, zero_start=False):
    """sum_p X[g][p][c] a[g][p]: PG row groups (rows pg, pg + PG, .. in turn, fma), the groups' partials added in order (zero_start:
    onto 0.f, the backward LDS kernel's loop; else onto the first partial)."""
    G, P, C = X.shape
    # fast path: the chain in numpy float64 (products exact), every sum kept; only if one of them sits on an fp32 midpoint (where the
    # rounding to 53 bits could have hidden on which side the true sum lies) the chain is redone with fma32's exact tie handling
    prod = (X.double() * a.double()[:, :, None]).numpy()
    acc, sums = np.zeros((G, PG, C)), np.empty((P, G, C))
    for p in range(P):
        sums[p] = prod[:, p] + acc[:, p % PG]
        acc[:, p % PG] = sums[p].astype(np.float32)
    if bool(((sums.view(np.int64) & ((1 << 29) - 1)) == (1 << 28)).any()):
        acc = torch.zeros(G, PG, C)
        for p in range(P):
            acc[:, p % PG] = fma32(X[:, p], a[:, p, None], acc[:, p % PG])
    else:
        acc = torch.from_numpy(acc).float()
    out = acc[:, 0] + 0.0 if zero_start else acc[:, 0].clone()
    for q in range(1, PG):
        out = out + acc[:, q]
    return out


def emu_softmax(s, form, PMAX=0):
    """scores [G][P] -> the fp32 weights.  form "block": the workgroup reduction of the plain and the LDS kernels; "seq": the register
    kernel's and cross attention's sum in index order."""
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    if form == "block":
        tot = emu_block_sum(e)
    else:
        tot = torch.zeros(s.shape[:-1])
        for p in range(s.shape[-1]):
            tot = tot + e[..., p]
    return e * (1.0 / tot).unsqueeze(-1)


def emu_attn_pool_fwd(X, w, b, kernel=None, mutant=None):
    """-> (attn, vec) in fp32 by the kernel the launcher takes at (P, C) (or the one named)."""
    G, P, C = X.shape
    kernel = kernel or fwd_kernel(P, C)
    bb = torch.tensor(0.0 if b is None else float(b))
    if kernel.startswith("attn_pool_fwd_reg"):
        s, PG, form = emu_dots_reg(X, w) + bb, 1, "seq"
    elif kernel == "attn_pool_fwd_lds_kernel":
        inner = fwd_lds_inner(P, C)
        s = (emu_dots_tpp(X, w.view(1, -1), inner["TPP"]) if inner["wide"] else emu_dots_wave(X, w.view(1, -1))) + bb
        PG, form = inner["PG"], "block"
    else:
        s, PG, form = emu_dots_wave(X, w.view(1, -1)) + bb, 1, "block"
    a = emu_softmax(s, form)
    if mutant == "wrong sum":            # normalised by the sum without the last point's term
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        a = e * (1.0 / (e.sum(-1, keepdim=True) - e[:, -1:]))
    return a, emu_colsum(X, a, PG)


def emu_da(X, dvec, kernel=None):
    """da[g][p] = x_p . dvec_g in fp32 by the kernel's form -> (da, PG of the dw partial sums)"""
    P, C = X.shape[1], X.shape[2]
    kernel = kernel or bwd_kernel(P, C)
    if kernel == "attn_pool_bwd_lds_kernel":
        inner = bwd_lds_inner(P, C)
        return (emu_dots_tpp(X, dvec, inner["TPP"]) if inner["wide"] else emu_dots_wave(X, dvec)), inner["PG"]
    return emu_dots_wave(X, dvec), 1


def emu_attn_pool_bwd(X, w, attn, dvec, kernel=None, mutant=None, dx_form=0):
    """-> (dX, pdw, pdb) in fp32, in the kernels' orders: da by emu_da, dot and pdb by the workgroup reduction, ds = attn (da - dot),
    pdw by PG row groups.  dX = attn dvec + ds w is one product and one fma; which product the compiler fuses the source does not
    fix: dx_form 0 is fma(attn, dvec, ds w), 1 is fma(ds, w, attn dvec)."""
    G, P, C = X.shape
    da, PG = emu_da(X, dvec, kernel)
    dot = emu_block_sum(attn, da)
    ds = attn * (da - dot[:, None])
    if mutant == "no dot":
        ds = attn * da
    pdb = emu_block_sum(ds)
    wv, dv = w.view(1, 1, C).expand(G, 1, C), dvec[:, None, :]
    if mutant == "swapped":
        wv, dv = dv, wv
    if dx_form == 0:
        dX = fma32(attn[:, :, None], dv, ds[:, :, None] * wv)
    else:
        dX = fma32(ds[:, :, None], wv, attn[:, :, None] * dv)
    return dX, emu_colsum(X, ds, PG, zero_start=True), pdb


def emu_cross_scores(A, B):
    """A [F][n][64] . B [F][m][64] by the scalar kernels' four lanes per row: 16 channels each in turn (fma), then shfl_xor 1 and 2."""
    F, n, m = A.shape[0], A.shape[1], B.shape[1]
    A4, B4 = A.view(F, n, 1, 4, 16), B.view(F, 1, m, 4, 16)
    d = torch.zeros(F, n, m, 4)
    for c in range(16):
        d = fma32(A4[..., c], B4[..., c], d)
    sub = torch.arange(4)
    d = d + d[..., sub ^ 1]
    d = d + d[..., sub ^ 2]
    return d[..., 0]


def emu_seq_matmul(A, B):
    """A [F][n][k] B [F][k][m], the k terms in index order (fma)."""
    acc = torch.zeros(A.shape[0], A.shape[1], B.shape[2])
    for j in range(A.shape[2]):
        acc = fma32(A[:, :, j, None], B[:, None, j, :], acc)
    return acc


def emu_cross_fwd(Q, K, V, scale, form="scalar"):
    """-> (P, O) in fp32.  "scalar": cross_attn_fwd_kernel's orders; "mfma": the matrix-pipe kernel, whose order inside an MFMA the source
    does not fix -- torch's fp32 products stand in for it."""
    if form == "scalar":
        S = emu_cross_scores(Q, K) * scale
        Pm = emu_softmax(S, "seq")
        return Pm, emu_seq_matmul(Pm, V)
    S = (Q @ K.transpose(1, 2)) * scale
    Pm = emu_softmax(S, "seq")
    return Pm, Pm @ V


def emu_rows_sum(X, scale, mutant=None):
    """group_sum_kernel: the P rows added in row order, then the product with scale.  X [G][P][C]"""
    P = X.shape[1]
    s = torch.zeros(X.shape[0], X.shape[2])
    for p in range(P):
        if mutant == "drops last" and P % 8 == 1 and p == P - 1:
            continue
        s = s + X[:, p]
    return s * torch.tensor(scale, dtype=torch.float32)


def emu_cross_bwd(Q, K, V, Pm, dO, scale, mutant=None):
    """cross_attn_bwd_kernel -> (dQ, dK, dV) in fp32"""
    dP = emu_cross_scores(dO, V)
    dot = torch.zeros(dP.shape[:2])
    for j in range(NK):
        dot = fma32(Pm[..., j], dP[..., j], dot)
    sc = torch.tensor(1.0 if mutant == "no scale" else scale, dtype=torch.float32)
    dS = Pm * (dP - dot[..., None]) * sc
    return emu_seq_matmul(dS, K), emu_seq_matmul(dS.transpose(1, 2).contiguous(), Q), emu_seq_matmul(Pm.transpose(1, 2).contiguous(), dO)


def emu_group_bcast(dY, P, scale, dX0=None):
    v = (dY * torch.tensor(scale, dtype=torch.float32))[:, None, :].expand(-1, P, -1)
    return v.clone() if dX0 is None else dX0 + v


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch mirrors (held to the text of pool.hip by test_pool_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def tile_nq(n4):
    """tile_to_lds_any's instantiation for a tile of n4 16-byte pieces."""
    nq = cdiv(n4, 256)
    return 2 if nq <= 2 else 4 if nq <= 4 else 8 if nq <= 8 else 16 if nq <= 16 else 24


def fwd_kernel(P, C, aligned=True):
    """mmego_attn_pool_forward's choice.  aligned: X, w and vec on 16-byte addresses."""
    tile = (P * C + P) * 4
    vec_ok = C % 4 == 0 and aligned
    if vec_ok and P <= 32 and C <= 1024:
        return "attn_pool_fwd_reg_kernel<20>" if P <= 20 else "attn_pool_fwd_reg_kernel<32>"
    if vec_ok and tile <= 96 * 1024:
        return "attn_pool_fwd_lds_kernel"
    return "attn_pool_fwd_kernel"


def fwd_lds_inner(P, C):
    """attn_pool_fwd_lds_kernel's work split at (P, C)."""
    TPP = 1
    while TPP * 2 * P <= 256 and TPP * 2 * P <= 1024 and C % (TPP * 2) == 0:
        TPP *= 2
    return {"TPP": TPP, "len": C // TPP, "wide": P * TPP <= 1024 and P <= 1024, "PG": 256 // C if (C <= 128 and 256 % C == 0) else 1,
            "wl": C <= 1024, "NQ": tile_nq(P * C // 4), "tile": (P * C + P) * 4, "lds": (P * C + P) * 4 + FWD_STATIC_LDS}


def bwd_tile(P, C):
    TCc = C if C < 256 else 256
    return (P * C + 2 * P + (256 // TCc) * C) * 4


def bwd_kernel(P, C, aligned=True):
    """mmego_attn_pool_backward's choice.  aligned: X on a 16-byte address."""
    TCc = C if C < 256 else 256
    if C % 4 == 0 and 256 % TCc == 0 and bwd_tile(P, C) <= 64 * 1024 and aligned:
        return "attn_pool_bwd_lds_kernel"
    return "attn_pool_bwd_kernel"


def bwd_lds_inner(P, C):
    """attn_pool_bwd_lds_kernel's work split at (P, C); "lds": the workgroup's whole group segment, static arrays included."""
    TPP = 1
    while TPP * 2 * P <= 256 and C % (TPP * 2) == 0:
        TPP *= 2
    TCc = C if C < 256 else 256
    return {"TPP": TPP, "len": C // TPP, "wide": P * TPP <= 1024, "TCc": TCc, "PG": 256 // TCc, "dl": C <= 1024, "NQ": tile_nq(P * C // 4),
            "tile": bwd_tile(P, C), "lds": bwd_tile(P, C) + BWD_STATIC_LDS}


def ew_blocks(total):
    return min(2048, max(1, cdiv(total, 256)))


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and cases shared by the GPU file and the CPU emulation test
# ---------------------------------------------------------------------------------------------------------------------------------
# (P, C, G, X one float past alignment) -> the kernel the case must reach
FWD_CASES = [(1, 4, 3, 0, "attn_pool_fwd_reg_kernel<20>"), (7, 36, 3, 0, "attn_pool_fwd_reg_kernel<20>"),
             (20, 1020, 3, 0, "attn_pool_fwd_reg_kernel<20>"), (20, 1024, 3, 0, "attn_pool_fwd_reg_kernel<20>"),
             (21, 64, 3, 0, "attn_pool_fwd_reg_kernel<32>"), (32, 1024, 3, 0, "attn_pool_fwd_reg_kernel<32>"),
             (33, 64, 3, 0, "attn_pool_fwd_lds_kernel"), (128, 64, 3, 0, "attn_pool_fwd_lds_kernel"), (100, 128, 3, 0, "attn_pool_fwd_lds_kernel"),
             (300, 12, 3, 0, "attn_pool_fwd_lds_kernel"), (5, 1028, 3, 0, "attn_pool_fwd_lds_kernel"), (1100, 8, 3, 0, "attn_pool_fwd_lds_kernel"),
             (96, 252, 3, 0, "attn_pool_fwd_lds_kernel"), (50, 30, 3, 0, "attn_pool_fwd_kernel"), (128, 256, 3, 0, "attn_pool_fwd_kernel"),
             (20, 64, 3, 1, "attn_pool_fwd_kernel"), (8192, 3, 1, 0, "attn_pool_fwd_kernel"),
             (7, 36, 1, 0, "attn_pool_fwd_reg_kernel<20>"), (7, 36, 257, 0, "attn_pool_fwd_reg_kernel<20>"),
             (33, 64, 1, 0, "attn_pool_fwd_lds_kernel"), (33, 64, 257, 0, "attn_pool_fwd_lds_kernel")]
BWD_CASES = [(1, 4, 3, 0, "attn_pool_bwd_lds_kernel"), (33, 16, 3, 0, "attn_pool_bwd_lds_kernel"), (128, 64, 3, 0, "attn_pool_bwd_lds_kernel"),
             (20, 256, 3, 0, "attn_pool_bwd_lds_kernel"), (1100, 8, 3, 0, "attn_pool_bwd_lds_kernel"), (120, 128, 3, 0, "attn_pool_bwd_lds_kernel"),
             (20, 1024, 3, 0, "attn_pool_bwd_kernel"), (40, 12, 3, 0, "attn_pool_bwd_kernel"), (50, 30, 3, 0, "attn_pool_bwd_kernel"),
             (128, 64, 3, 1, "attn_pool_bwd_kernel")]
CROSS_F = (1, 3, 37)
POOLED_Q_F = 2051            # past the persistent launch's 2048 workgroups: workgroups 0..2 walk on to frames 2048..2050
SUM_P = (1, 7, 8, 9, 15, 64)
SUM_GC = ((3, 5), (4, 64), (1, 256), (1, 257))
BCAST_BIG = (33, 64, 256)    # G, P, C: 540,672 elements, past 2048 blocks of 256


def shifts(G, kinds=5):
    """The row-kind shifts a case of G groups runs at so that every kind occurs, and at least one even shift (b given) and one odd
    (b == NULL)."""
    return tuple(range(0, kinds, G)) if G < kinds else (0, 1)


def pool_inputs(G, P, C, shift=0):
    """X [G][P][C], w [C], b (None at odd shifts), dvec [G][C].  Group g is of kind (g + shift) % 5: 0 ordinary (scores of order 1), 1 one
    score ahead by 30, 2 one ahead by 200 (weights exactly 0 and 1), 3 tied (one non-zero channel, the same in every row: the score is
    one exact product in every summation order, attn == 1 / P), 4 all scores near -100."""
    g = gen_for(71, G, P, C, shift)
    X, w = torch.randn(G, P, C, generator=g), torch.randn(C, generator=g) / C ** 0.5
    b = None if shift % 2 else float(torch.randn(1, generator=g)) * 0.5
    u = w / float((w.double() ** 2).sum())
    kinds = (torch.arange(G) + shift) % 5
    for gi in range(G):
        k, ps = int(kinds[gi]), (7 * gi + 3) % P
        if k == 1:
            X[gi, ps] += 30.0 * u
        elif k == 2:
            X[gi, ps] += 200.0 * u
        elif k == 3:
            X[gi] = 0.0
            X[gi, :, (5 * gi + 1) % C] = 1.5
        elif k == 4:
            X[gi] += -100.0 * u
    return {"X": X, "w": w, "b": b, "dvec": torch.randn(G, C, generator=g), "kinds": kinds}


def cross_inputs(F, shift=0, proj=False):
    """Q [F][64][64], K, V [F][15][64], dO.  Channel 0 of every query is 4, so a key's channel 0 moves all of its scores together:
    frame f is of kind (f + shift) % 8: 0, 6 ordinary, 1 key 14 ahead by 30, 2 key 0 ahead by 30, 3 a key ahead by 200, 4 tied (all keys
    equal), 5 all scores near -100, 7 key 14 ahead by 200.  proj: X, Wq, bq with Q = X Wq^T + bq (Wq's row 0 is zero and bq[0] = 4)."""
    g = gen_for(72, F, shift, int(proj))
    scale = 0.125
    r = {"scale": scale, "kinds": (torch.arange(F) + shift) % 8}
    if proj:
        r["X"], r["Wq"], r["bq"] = torch.randn(F, NQ, DH, generator=g), torch.randn(DH, DH, generator=g) / 8.0, torch.randn(DH, generator=g) * 0.3
        r["Wq"][0], r["bq"][0] = 0.0, 4.0
    else:
        r["Q"] = torch.randn(F, NQ, DH, generator=g)
        r["Q"][:, :, 0] = 4.0
    K, V = torch.randn(F, NK, DH, generator=g), torch.randn(F, NK, DH, generator=g)
    for f in range(F):
        k = int(r["kinds"][f])
        lead = {1: (14, 30.0), 2: (0, 30.0), 3: ((3 * f + 5) % NK, 200.0), 7: (14, 200.0)}.get(k)
        if lead:
            K[f, lead[0], 0] += lead[1] / (scale * 4.0)
        elif k == 4:
            K[f] = K[f, 0].clone()
        elif k == 5:
            K[f, :, 0] += -100.0 / (scale * 4.0)
    r["K"], r["V"], r["dO"] = K, V, torch.randn(F, NQ, DH, generator=g)
    return r


def half_attn(G, P):
    """attn with one non-zero entry per group, 0.5 at row ps[g]: dot = da / 2 and ds = da / 4 there, exactly, and pdb = da[ps] / 4 --
    the bits of one da, the TPP partial sums in their order, seen from outside."""
    ps = (11 * torch.arange(G) + 5) % P
    a = torch.zeros(G, P)
    a[torch.arange(G), ps] = 0.5
    return a, ps


def sum_inputs(G, P, C, key=0):
    g = gen_for(73, G, P, C, key)
    return torch.randn(G, P, C, generator=g), torch.randn(G, C, generator=g)
