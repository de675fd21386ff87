"""Plain float64 restatements of the fused ST-GCN training kernels (csrc/gcn_fused.hip and the record-carrying temporal convolutions of
csrc/gcn.hip) with a-priori fp32 rounding bounds, for tests/test_gcn_train_gpu.py.  Every function takes the fp32 values a kernel read
(CPU tensors) and returns (reference, bound) pairs in float64; |out - ref| <= MARGIN * bound is what the tests assert.

Bound forms (the ones of tests/test_mlp_train_gpu.py):
  products                  (n + c) 2^-24 sum |a| |b|: n the accumulation chain, c the roundings in front of the product
  fp64-accumulated sums     n 2^-53 sum |summand| plus the fp32 roundings of summand and result
  fp32-accumulated records  the fp32 chain length (the rows of the record: every row part's chain plus the parts' additions is shorter)
Magnitudes inside a bound always come from the float64 reference of the quantity (upper()), never from the kernel's output."""
import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53
MARGIN = 4.0            # tests/test_mlp_train_gpu.py's: for what the bounds do not model (1 / sqrt, casts, second-order terms)
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))
MOM = float(torch.tensor(0.1, dtype=torch.float32))
# dz = a (g - c1 - xhat c2): x - mu, * is, * c2, g - c1, the second subtraction, a *, and the fp32 roundings of c1 and c2
CDZ = 8
# act(x) = max(fmaf(x - mu, a, b), 0): the subtraction and the fma, relative to |x - mu| |a| + |b|
CACT = 2
# x = max(fmaf(x1 - m1, a1, b1) + fmaf(x2 - m2, a2, b2), 0): two roundings per branch, each relative to its own magnitude, and the sum
CPAIR = 3


def upper(ref, bound):
    """Ceiling of |out| for an output that passed check(out, ref, bound)."""
    return ref.abs() + MARGIN * bound


def groups(rows, rpr):
    """(first row, row count) of the records of `rows` rows at rpr rows per record (the last one ragged)."""
    return [(s, min(rpr, rows - s)) for s in range(0, rows, rpr)]


def make_records(x, rows_per_rec):
    """(mean, M2) records [nrec][C][2] of x [rows][C] in fp64, rounded to fp32: what a producer kernel would have left."""
    out = []
    for s, n in groups(x.shape[0], rows_per_rec):
        xs = x[s:s + n].double()
        m = xs.mean(0)
        out.append(torch.stack((m, ((xs - m) ** 2).sum(0)), 1))
    return torch.stack(out).float()


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm state and running statistics from partial records (gcn_stats.h bn_gather / bn_finish)
# ---------------------------------------------------------------------------------------------------------------------------------
def stats_from_records(rec, rows, rpr, gamma, beta, rm0, rv0):
    """rec [nrec][C][2] fp32 -> state [4][C] (mean, invstd, a, b), its bound, and torch's running-statistics update (momentum, unbiased
    variance; N = 1: the biased one) with bounds.  mean, invstd: one fp32 rounding of the fp64 value; a = gamma invstd: two; behind them
    the fp64 error of the nrec-term sums and of the cancellation in M2 = sum M2_j + sum n_j mean_j^2 - N mean^2."""
    r = rec.double()
    n = torch.tensor([g[1] for g in groups(rows, rpr)], dtype=torch.float64).view(-1, 1)
    assert n.shape[0] == r.shape[0], (n.shape, r.shape)
    nrec, N = r.shape[0], float(rows)
    m = (n * r[:, :, 0]).sum(0) / N
    SS = (n * r[:, :, 0] ** 2).sum(0)
    M2 = (r[:, :, 1].sum(0) + SS - N * m * m).clamp_min(0.0)
    var = M2 / N
    istd = 1.0 / torch.sqrt(var + EPS32)
    e_m = (nrec + 1) * U64 * (n * r[:, :, 0].abs()).sum(0) / N
    e_var = (nrec + 4) * U64 * (r[:, :, 1].sum(0) + SS + N * m * m) / N
    b_istd = U32 * istd + 0.5 * istd ** 3 * e_var
    a = gamma.double() * istd
    state = torch.stack((m, istd, a, beta.double()))
    bound = torch.stack((U32 * m.abs() + e_m, b_istd, gamma.abs().double() * b_istd + U32 * a.abs(), torch.zeros_like(m)))
    out = {"state": (state, bound)}
    if rm0 is not None:
        unb = M2 / (N - 1.0) if N > 1 else var
        k = N / (N - 1.0) if N > 1 else 1.0
        rm = (1 - MOM) * rm0.double() + MOM * m
        rv = (1 - MOM) * rv0.double() + MOM * unb
        out["rm"] = (rm, U32 * (2 * ((1 - MOM) * rm0.double()).abs() + 2 * (MOM * m).abs() + rm.abs()) + MOM * e_m)
        out["rv"] = (rv, U32 * (2 * ((1 - MOM) * rv0.double()).abs() + 2 * MOM * unb + rv.abs()) + MOM * e_var * k)
    return out


def stats_direct(x, gamma, beta, rm0, rv0, chain):
    """data_bn inside gcn_front (in_mode 0): statistics of x [N][C] taken by the kernel itself -- per thread an fp32 chain of `chain` shifted
    values (shift = row 0), the eight row groups added in fp64."""
    xd = x.double()
    N = xd.shape[0]
    d = xd - xd[0]
    S1, S2 = d.sum(0), (d * d).sum(0)
    m = xd[0] + S1 / N
    M2 = (S2 - S1 * S1 / N).clamp_min(0.0)
    var = M2 / N
    istd = 1.0 / torch.sqrt(var + EPS32)
    Dabs, D2 = d.abs().sum(0), S2
    e_m = U32 * (chain + 2) * Dabs / N
    e_var = U32 * (3 * chain + 14) * D2 / N
    b_istd = U32 * istd + 0.5 * istd ** 3 * e_var
    a = gamma.double() * istd
    state = torch.stack((m, istd, a, beta.double()))
    bound = torch.stack((U32 * m.abs() + e_m, b_istd, gamma.abs().double() * b_istd + U32 * a.abs(), torch.zeros_like(m)))
    out = {"state": (state, bound)}
    if rm0 is not None:
        unb = M2 / (N - 1.0) if N > 1 else var
        k = N / (N - 1.0) if N > 1 else 1.0
        rm = (1 - MOM) * rm0.double() + MOM * m
        rv = (1 - MOM) * rv0.double() + MOM * unb
        out["rm"] = (rm, U32 * (2 * ((1 - MOM) * rm0.double()).abs() + 2 * (MOM * m).abs() + rm.abs()) + MOM * e_m)
        out["rv"] = (rv, U32 * (2 * ((1 - MOM) * rv0.double()).abs() + 2 * MOM * unb + rv.abs()) + MOM * e_var * k)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# (mean, M2) records a kernel derives from an output tile of its own (tile_records, the tconv epilogues): fp32 shifted sums
# ---------------------------------------------------------------------------------------------------------------------------------
def records_of(own, ref, bound, grp):
    """own [rows][C]: the kernel's own fp32 output (the records are derived from it); ref, bound: the float64 reference that output was
    held to -- every magnitude below comes from them.  Per record of n rows with shift = its first row and d = x - shift:
      mean = shift + sum d / n     n - 1 additions of values rounded once, the division, the final addition: (n + 3) u sum|d| / n + u |mean|
      M2   = sum d^2 - (sum d)^2/n d^2 carries 2 u, the fma chain n u, the product s1 md 2 (n + 3) u + 3 u of (sum|d|)^2 / n <= sum d^2, the
                                   subtraction u (sum d^2 + (sum d)^2 / n): (3 n + 14) u sum d^2
    -> rec [ng][C][2], bound [ng][C][2]."""
    own, ref, bound = own.double(), ref.double(), bound.double().expand_as(ref)
    recs, bnds = [], []
    for s, n in grp:
        x = own[s:s + n]
        d = x - x[0]
        S1 = d.sum(0)
        mean, M2 = x[0] + S1 / n, ((d * d).sum(0) - S1 * S1 / n).clamp_min(0.0)
        dm = (ref[s:s + n] - ref[s]).abs() + MARGIN * (bound[s:s + n] + bound[s])
        dm[0] = 0.0                                               # (x[0] - x[0] is exact)
        Dabs, D2 = dm.sum(0), (dm * dm).sum(0)
        recs.append(torch.stack((mean, M2), 1))
        bnds.append(torch.stack((U32 * ((n + 3) * Dabs / n + upper(ref[s], bound[s]) + Dabs / n), U32 * (3 * n + 14) * D2), 1))
    return torch.stack(recs), torch.stack(bnds)


# ---------------------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_parts(z, st):
    """z [rows][C] fp32, st [4][C] fp32 (mean, invstd, a, b) -> the kernel's mask fmaf(z - mean, a, b) > 0 exactly (fp32 subtraction, then
    a product of two fp32 numbers is exact in fp64 and the addition cannot change a sign); bn(z), its magnitude |z - mean| |a| + |b|,
    |z - mean| |a| and xhat = (z - mean) invstd in fp64."""
    mean, istd, a, b = st[0], st[1], st[2], st[3]
    if z.dtype == torch.float32:
        mask = ((z - mean).double() * a.double() + b.double()) > 0
    else:
        mask = ((z - mean) * a + b) > 0
    d = z.double() - mean.double()
    da = d.abs() * a.abs().double()
    return mask, d * a.double() + b.double(), da + b.abs().double(), da, d * istd.double()


def pair_act(x1, st1, x2, st2):
    """x = max(bn1(x1) + bn2(x2), 0) (continuous in its argument: no mask), its magnitude and the roundings in front (CPAIR)."""
    _, v1, m1, _, _ = bn_parts(x1, st1)
    _, v2, m2, _, _ = bn_parts(x2, st2)
    return (v1 + v2).clamp_min(0.0), m1 + m2, CPAIR


def product(x, xmag, cx, W, bias):
    """Z = x W^T (+ bias) and its bound: cin accumulated terms, cx roundings in front, one for the bias; also the magnitude."""
    Wd = W.double()
    z, zm, c = x @ Wd.t(), xmag @ Wd.abs().t(), cx
    if bias is not None:
        z, zm, c = z + bias.double(), zm + bias.abs().double(), c + 1
    return z, (W.shape[1] + c) * U32 * zm


def einsum_mix(zref, zbound, A, imp, F, V, K, cout):
    """Y[f, w, c] = sum_k sum_v (A . imp)[k, v, w] z[f, v, k cout + c] from the float64 reference of z: the error z carries goes through
    |A . imp|; on top the product's own chain (<= 16 K terms on 16x16x4 MFMAs) and the fp32 rounding of A . imp."""
    ae = A.double() * imp.double()
    z4, b4 = zref[:, :K * cout].reshape(F, V, K, cout), zbound[:, :K * cout].reshape(F, V, K, cout)
    y = torch.einsum("kvw,fvkc->fwc", ae, z4)
    ymag = torch.einsum("kvw,fvkc->fwc", ae.abs(), z4.abs())
    yb = torch.einsum("kvw,fvkc->fwc", ae.abs(), b4) + (16 * K + 1) * U32 * ymag
    return y.reshape(F * V, cout), yb.reshape(F * V, cout)


# ---------------------------------------------------------------------------------------------------------------------------------
# temporal convolution
# ---------------------------------------------------------------------------------------------------------------------------------
def tconv(act, amag, ca, W, bias, B, T, V):
    """Y[r][co] = bias[co] + sum_tap sum_ci act[r + (tap - half) V][ci] W[co][ci][tap], frames outside the sequence contribute nothing.
    Bound: taps * Cin accumulated terms, up to three additions of the step groups' partial tiles, ca roundings in front, the bias."""
    Co, Ci, taps = W.shape
    rows, half = B * T * V, taps // 2
    a4, m4 = act.reshape(B, T, V, Ci), amag.reshape(B, T, V, Ci)
    y, ym = act.new_zeros(rows, Co), act.new_zeros(rows, Co)
    Wd = W.double()
    for tap in range(taps):
        d = tap - half
        if abs(d) >= T:
            continue
        sa, sm = torch.zeros_like(a4), torch.zeros_like(m4)
        if d >= 0:
            sa[:, :T - d], sm[:, :T - d] = a4[:, d:], m4[:, d:]
        else:
            sa[:, -d:], sm[:, -d:] = a4[:, :T + d], m4[:, :T + d]
        y += sa.reshape(rows, Ci) @ Wd[:, :, tap].t()
        ym += sm.reshape(rows, Ci) @ Wd[:, :, tap].abs().t()
    c = ca + 3
    if bias is not None:
        y, ym, c = y + bias.double(), ym + bias.abs().double(), c + 1
    return y, (taps * Ci + c) * U32 * ym


def tconv_input_grad(dy, W, B, T, V):
    """dAct[r][ci] = sum_tap sum_co dY[r - (tap - half) V][co] W[co][ci][tap]: the same convolution with the transposed, tap-reversed weight."""
    return tconv(dy.double(), dy.abs().double(), 0, W.permute(1, 0, 2).flip(2).contiguous(), None, B, T, V)


def g_records(own, ref, bound, ym, st, grp, mask=None):
    """bw_rec / gcn_bn_bwd_reduce records: (sum g, sum g xhat) per record, g = own . mask in fp32 chains of at most n terms.  own: the fp32
    gradient the sums are taken of (an input, or the kernel's own output held to (ref, bound) -- the magnitudes come from those);
    mask: the kernel's own decision by the sign identity unless given (an input tensor).  s2's summand carries three fp32 roundings
    (x - mu, * is, g *)."""
    m, _, _, _, xhat = bn_parts(ym, st)
    if mask is None:
        mask = m
    g = own.double() * mask
    gm = upper(ref.double(), bound.double().expand_as(ref)) * mask
    recs, bnds = [], []
    for s, n in grp:
        gs, xs, ms = g[s:s + n], xhat[s:s + n], gm[s:s + n]
        a2 = (ms * xs.abs()).sum(0)
        recs.append(torch.stack((gs.sum(0), (gs * xs).sum(0)), 1))
        bnds.append(torch.stack((n * U32 * ms.sum(0), (n + 3) * U32 * a2), 1))
    return torch.stack(recs), torch.stack(bnds)


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm backward from (sum g, sum g xhat) records
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_bwd(g, x, st, rec, rows):
    """rec [nrec][C][2] fp32 (sum g, sum g xhat); g [rows][C] the masked gradient (float64 values of fp32 numbers).
    -> d(beta), d(gamma) (fp64 sums of the records rounded once) and dX = a (g - c1 - xhat c2) with its magnitude."""
    r = rec.double()
    S1, S2 = r[:, :, 0].sum(0), r[:, :, 1].sum(0)
    eS = r.shape[0] * U64
    xhat = bn_parts(x, st)[4]
    a = st[2].double()
    c1, c2 = S1 / rows, S2 / rows
    dx = a * (g - c1 - xhat * c2)
    dxm = a.abs() * (g.abs() + c1.abs() + (xhat * c2).abs())
    return {"dbeta": (S1, U32 * S1.abs() + eS * r[:, :, 0].abs().sum(0)), "dgamma": (S2, U32 * S2.abs() + eS * r[:, :, 1].abs().sum(0)),
            "dX": (dx, CDZ * U32 * dxm), "dXmag": dxm}


def graph_dA(z, dy, dymag, A, imp, G, V, K, C, fpb=2):
    """dZ[g, v, k C + c] = sum_w (A . imp)[k, v, w] dy[g, w, c] and, per workgroup of fpb frames, partial[k, v, w] = sum_g sum_c z[g, v, k C
    + c] dy[g, w, c]; dy carries CDZ roundings relative to dymag.  Chains: 16 terms (+ the rounding of A . imp) and fpb C terms."""
    ae = A.double() * imp.double()
    d4, m4, z4 = dy.reshape(G, V, C), dymag.reshape(G, V, C), z.double().reshape(G, V, K, C)
    dz = torch.einsum("kvw,gwc->gvkc", ae, d4).reshape(G * V, K * C)
    dzm = torch.einsum("kvw,gwc->gvkc", ae.abs(), m4).reshape(G * V, K * C)
    nblk = (G + fpb - 1) // fpb
    part, pm = z.new_zeros((nblk, K, V, V), dtype=torch.float64), z.new_zeros((nblk, K, V, V), dtype=torch.float64)
    for j in range(nblk):
        sl = slice(j * fpb, min(G, (j + 1) * fpb))
        part[j] = torch.einsum("gvkc,gwc->kvw", z4[sl], d4[sl])
        pm[j] = torch.einsum("gvkc,gwc->kvw", z4[sl].abs(), m4[sl])
    return {"dZ": (dz, (16 + 1 + CDZ) * U32 * dzm), "partial": (part, (fpb * C + CDZ) * U32 * pm)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference block of the chain test, with torch ops (float64 autograd runs through it)
# ---------------------------------------------------------------------------------------------------------------------------------
def bn_train(x, gamma, beta):
    return (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + EPS32) * gamma + beta


def block_torch(x, P, A, imp, B, T, V, K, cout, masks=None):
    """st_gcn block on channels-last rows (b, t, v): 1x1 conv -> einsum with A . importance -> BN -> ReLU -> 9x1 conv -> BN, + residual (1x1
    conv -> BN), ReLU.  P: dict of float64 parameters.  masks = (m0, mout) replaces the two ReLUs by multiplications.  -> out and the
    intermediate tensors."""
    F, rows, cin = B * T, B * T * V, x.shape[1]
    zr = x @ P["Wc"].t() + P["bc"]
    z, rz = zr[:, :K * cout], zr[:, K * cout:]
    ymix = torch.einsum("kvw,fvkc->fwc", A * imp, z.reshape(F, V, K, cout)).reshape(rows, cout)
    h0 = bn_train(ymix, P["g0"], P["b0"])
    y0 = h0 * masks[0] if masks is not None else torch.relu(h0)
    yc = y0.reshape(B, T * V, cout).transpose(1, 2).reshape(B, cout, T, V)
    tz = torch.nn.functional.conv2d(yc, P["Wt"].reshape(cout, cout, 9, 1), P["bt"], padding=(4, 0))
    tz = tz.reshape(B, cout, T * V).transpose(1, 2).reshape(rows, cout)
    pre = bn_train(tz, P["g3"], P["b3"]) + bn_train(rz, P["gr"], P["br"])
    out = pre * masks[1] if masks is not None else torch.relu(pre)
    return out, {"zr": zr, "ymix": ymix, "y0": y0, "tz": tz, "h0": h0, "pre": pre}
