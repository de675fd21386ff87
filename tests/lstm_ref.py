"""Plain float64 restatements of the LSTM recurrence kernels (csrc/lstm.hip, lstm_step.hip, lstm_bwd_step.hip, the K-quartered backward
step of gemm.hip, the stage-1 pieces of imu_train.hip; one cell: csrc/lstm_cell.h, PyTorch gate order i, f, g, o) with a-priori fp32
rounding bounds, for tests/test_lstm_kernels_gpu.py and tests/test_lstm_ref_cpu.py.  Every function takes the fp32 values a kernel read
(CPU tensors) and returns (reference, bound) pairs in float64; |out - ref| <= MARGIN * bound elementwise is what the GPU tests assert, and
an fp32 emulation of the same expressions (emu_* below) has to stay inside the bounds WITHOUT the margin (test_lstm_ref_cpu.py).

u = 2^-24 (one fp32 rounding, relative).  Bound forms, all first order (what they leave out -- second-order terms, the slope of an
activation changing inside the error interval -- is what MARGIN = 4 is for, as in tests/gcn_train_ref.py):

  pre-activation   p = xproj + b_hh + sum_k h_k W_k:  (K + c) u (|xproj| + |b_hh| + sum |h_k| |W_k|)  [+ sum e(h_k) |W_k| in a chain]
                   K the accumulation chain (H: the MFMA accumulator takes every k in turn; a kernel that splits the chain in two
                   has shorter chains and one more addition), c the additions in front of and behind the product, per kernel:
                     lstm64 forward      acc + (xp + b)                  c = 2
                     lstm_step_dma       accumulators seeded with xp + b c = 1
                     lstm_step_small     acc0 + acc1 + (xp + b)          c = 3
                     lstm_first_step     xp + b, no product              c = 1, K = 0
  fast activations (lstm_cell.h): sigmoid(x) = rcp(1 + exp2(x' L)), x' = -x, L = fp32(log2 e).
                   ASSUMPTION: v_exp_f32 and v_rcp_f32 are accurate to 1 ulp (2 u relative at worst).  No ISA document is part of this
                   tree; 1 ulp is what the public CDNA ISA guides state for both.
                     e = exp2(fl(x' L)):  the product's rounding (u) and the constant's own (|L - log2 e| / log2 e = 0.224 u) are
                        relative errors of the ARGUMENT: times |x' log2 e| ln 2 = |x| they are relative errors of e;  + 2 u (v_exp)
                        rel(e) = 1.224 |x| u + 2 u
                     d = fl(1 + e): u;   r = rcp(d): 2 u;   d ln s / d ln e = -(1 - s):
                        rel(s) = (1 - s) rel(e) + 3 u                                     RELATIVE in s
                   Past |x| = 88.7 exp overflows (s = 0 where sigmoid < 2^-126) or underflows (s = 1): every bound carries the
                   absolute floor TINY = 2^-126, below which fp32 results are denormal (quantised at 2^-149, or flushed).
                   tanh(x) = 1 - 2 r, r = sigmoid(-2x) by the same instructions (2x and 2r are exact):
                        abs(t) = 2 r rel(r) + u |t|                                       ABSOLUTE: 4 u at x = 0, where t = 1 - 2r cancels
                   libm tanhf (the stage-1 backward kernels): TANHF_ULP = 5 ulp relative, the bound OpenCL's full profile sets for tanh
                   and OCML is built to; no document in this tree gives a tighter one.
                   An argument known to e(x) adds |f'(x)| e(x): s (1 - s) e(x), (1 - t^2) e(x).
  cell update      c = f c_prev + i g (one product rounded, then an fma, in either order): u |f c_prev| + u |i g| + u |c|, plus
                   e(f) |c_prev| + f e(c_prev) + e(i) |g| + i e(g);   h = o tanh(c): u |h| + e(o) |tanh c| + o e(tanh c), e(tanh c)
                   the fast form's absolute error plus (1 - tanh^2 c) e(c).
  cell backward    (lstm_cell_bwd) one rounding per operation, relative to its own term; the stashed gates are INPUTS (exact):
                     q = 1 - tc^2:   u tc^2 + u |q| + 2 |tc| e(tc)
                     m = dh go q:    2 u |m| + |dh go| e(q) + |go q| e(dh)
                     dcv = dc + m:   u |dcv| + e(dc) + e(m)
                     di = dcv gg gi (1 - gi), df = dcv cprev gf (1 - gf):   4 u |.| + e(dcv) |the other factors|
                     dg = dcv gi (1 - gg^2):   |dcv gi| (u gg^2 + u |1 - gg^2|) + 2 u |dg| + e(dcv) |gi (1 - gg^2)|
                     do = dh tc go (1 - go):   4 u |do| + e(dh) |tc go (1 - go)| + e(tc) |dh go (1 - go)|
                     dcprev = dcv gf:          u |dcprev| + e(dcv) gf
                   dh = dout + dh_rec: u |dh| + e(dh_rec).
  dh_rec products  (4H + c) u sum |dg_n| |W_nk| [+ sum e(dg_n) |W_nk|]: chain 256 for the H = 64 pair (four chains of 64 and their
                   (a0 + a1) + (a2 + a3): c = 2), 4H for lstm_bwd_step (c = 0; the K-quartered form adds its four quarters: c = 3).
  chains           a recurrence whose intermediate state cannot be observed (lstm64 forward without stashes, all of lstm64 backward)
                   carries e(h), e(c) / e(dc), e(dgates) beside the values through the steps by the rules above.  With stashes the
                   test checks step by step from the kernel's OWN fp32 h_{t-1} and c_{t-1}: no amplification.
  loss and head    (imu_loss, imu_head, imu_head_backward) a running error analysis: class EB carries a first-order bound beside each
                   float64 value through the kernel's own operations; the reference values are float64 autograd of the restated forward.
Magnitudes inside a bound always come from the float64 reference."""
import math

import torch

U32 = 2.0 ** -24
MARGIN = 4.0            # tests/gcn_train_ref.py's
TINY = 2.0 ** -126
ULP = 2.0 * U32         # 1 ulp, relative, at worst
EXP_ULP = 1.0
RCP_ULP = 1.0
TANHF_ULP = 5.0
LOG2E = math.log2(math.e)
LOG2E32 = float(torch.tensor(LOG2E, dtype=torch.float32))
C_L2E = abs(LOG2E32 - LOG2E) / LOG2E / U32       # 0.224
C_PRE = {"lstm64": 2, "dma": 1, "small": 3, "first": 1}


def D(t):
    return None if t is None else t.double()


# ---------------------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------------------
def _rel_sig(x):
    """relative error of rcp(1 + exp2(fl(-x L)))"""
    return torch.sigmoid(-x) * (x.abs() * (C_L2E + 1.0) * U32 + EXP_ULP * ULP) + U32 + RCP_ULP * ULP


def sigmoid(x, ex=0.0):
    s = torch.sigmoid(x)
    return s, s * _rel_sig(x) + s * (1 - s) * ex + TINY


def tanh_fast(x, ex=0.0):
    t, r = torch.tanh(x), torch.sigmoid(-2 * x)
    return t, 2 * r * _rel_sig(-2 * x) + U32 * t.abs() + (1 - t * t) * ex + 2 * TINY


def tanh_libm(x, ex=0.0):
    t = torch.tanh(x)
    return t, TANHF_ULP * ULP * t.abs() + (1 - t * t) * ex + TINY


# ---------------------------------------------------------------------------------------------------------------------------------
# cell
# ---------------------------------------------------------------------------------------------------------------------------------
def cell_fwd(P, eP, cprev, ec=0.0, first=False):
    """P, eP: pre-activations [.., 4, H] and their bound; cprev [.., H] (None: 0) -> {i, f, g, o, c, h: (ref, bound)}.  first: the
    first-step kernel forms c = i g alone."""
    i, ei = sigmoid(P[..., 0, :], eP[..., 0, :])
    f, ef = sigmoid(P[..., 1, :], eP[..., 1, :])
    g, eg = tanh_fast(P[..., 2, :], eP[..., 2, :])
    o, eo = sigmoid(P[..., 3, :], eP[..., 3, :])
    if cprev is None or first:
        c = i * g
        e_c = U32 * c.abs() + ei * g.abs() + i * eg + TINY
    else:
        c = f * cprev + i * g
        e_c = U32 * ((f * cprev).abs() + (i * g).abs() + c.abs()) + ef * cprev.abs() + f * ec + ei * g.abs() + i * eg + TINY
    tc, etc = tanh_fast(c, e_c)
    h = o * tc
    e_h = U32 * h.abs() + eo * tc.abs() + o * etc + TINY
    return {"i": (i, ei), "f": (f, ef), "g": (g, eg), "o": (o, eo), "c": (c, e_c), "h": (h, e_h)}


def cell_bwd(gi, gf, gg, go, c, cprev, dc, dh, e_dc=0.0, e_dh=0.0, tanh="libm"):
    """lstm_cell_bwd on stashed gates (inputs), tc = tanh(c) by the kernel's form -> {di, df, dg, do, dcprev: (ref, bound)}."""
    gi, gf, gg, go, c, dc, dh = (D(v) for v in (gi, gf, gg, go, c, dc, dh))
    cprev = torch.zeros_like(c) if cprev is None else D(cprev)
    tc, etc = (tanh_libm if tanh == "libm" else tanh_fast)(c)
    q = 1 - tc * tc
    eq = U32 * tc * tc + U32 * q.abs() + 2 * tc.abs() * etc
    m = dh * go * q
    em = 2 * U32 * m.abs() + (dh * go).abs() * eq + (go * q).abs() * e_dh
    dcv = dc + m
    edcv = U32 * dcv.abs() + e_dc + em
    ki, kf = gg * gi * (1 - gi), cprev * gf * (1 - gf)
    di, df = dcv * ki, dcv * kf
    qg = 1 - gg * gg
    dg = dcv * gi * qg
    ko = go * (1 - go)
    do = dh * tc * ko
    dcp = dcv * gf
    return {"di": (di, 4 * U32 * di.abs() + edcv * ki.abs() + TINY),
            "df": (df, 4 * U32 * df.abs() + edcv * kf.abs() + TINY),
            "dg": (dg, (dcv * gi).abs() * U32 * (gg * gg + qg.abs()) + 2 * U32 * dg.abs() + edcv * (gi * qg).abs() + TINY),
            "do": (do, 4 * U32 * do.abs() + e_dh * (tc * ko).abs() + etc * (dh * ko).abs() + TINY),
            "dcprev": (dcp, U32 * dcp.abs() + edcv * gf + TINY)}


def dgates_of(r):
    """cell_bwd's four gate gradients as [.., 4H] (gate-major columns) reference and bound."""
    return (torch.cat([r[k][0] for k in ("di", "df", "dg", "do")], -1), torch.cat([r[k][1] for k in ("di", "df", "dg", "do")], -1))


# ---------------------------------------------------------------------------------------------------------------------------------
# one step
# ---------------------------------------------------------------------------------------------------------------------------------
def preact(xp, b, hprev, W, cadd, eh=None):
    """xp [B][4H] (gate-major columns), b [4H] or None, hprev [B][H] or None (first step), W [4H][H] -> (P, bound) [B][4][H]."""
    xp = D(xp)
    B, H = xp.shape[0], xp.shape[1] // 4
    P, mag, K, prop = xp.clone(), xp.abs(), 0, 0.0
    if b is not None:
        P, mag = P + D(b), mag + D(b).abs()
    if hprev is not None:
        P, mag, K = P + D(hprev) @ D(W).t(), mag + D(hprev).abs() @ D(W).abs().t(), H
        if eh is not None:
            prop = eh @ D(W).abs().t()
    return P.view(B, 4, H), ((K + cadd) * U32 * mag + prop).view(B, 4, H)


def step(xp, b, hprev, W, cprev, kind, eh=None, ec=0.0):
    """One step: {gates [B][4H], c, h: (ref, bound)}.  kind: key of C_PRE (which kernel's additions); "first": no product, c = i g."""
    first = kind == "first"
    P, eP = preact(xp, b, None if first else hprev, W, C_PRE[kind], eh)
    r = cell_fwd(P, eP, None if first else D(cprev), ec, first)
    r["gates"] = (torch.cat([r[k][0] for k in "ifgo"], -1), torch.cat([r[k][1] for k in "ifgo"], -1))
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# whole bidirectional sequence (any H; the kernels: H = 64), forward and backward, bounds chained
# ---------------------------------------------------------------------------------------------------------------------------------
def seq_fwd(xp, W, b, h0, c0, kind="lstm64"):
    """xp[d] [B][T][4H], W[d] [4H][H], b[d] [4H] or None, h0[d] / c0[d] [B][H] or None.  Direction 1 walks t = T-1 .. 0.
    -> dict: out [B][T][2H], hn / cn [2][B][H] as (ref, bound) with the error carried through the steps; gates[d] [T][B][H][4],
    cst[d] [T][B][H], hprev[d] [B][T][H]: the float64 stashes (references only)."""
    B, T, H = xp[0].shape[0], xp[0].shape[1], xp[0].shape[2] // 4
    out, eout = torch.zeros(B, T, 2 * H, dtype=torch.float64), torch.zeros(B, T, 2 * H, dtype=torch.float64)
    res = {"gates": [], "cst": [], "hprev": [], "hn": [], "cn": []}
    for d in range(2):
        h = torch.zeros(B, H, dtype=torch.float64) if h0[d] is None else D(h0[d])
        c = torch.zeros(B, H, dtype=torch.float64) if c0[d] is None else D(c0[d])
        eh, ec = torch.zeros_like(h), torch.zeros_like(c)
        gates, cst, hprev = torch.zeros(T, B, H, 4, dtype=torch.float64), torch.zeros(T, B, H, dtype=torch.float64), torch.zeros(B, T, H, dtype=torch.float64)
        for s in range(T):
            t = s if d == 0 else T - 1 - s
            hprev[:, t] = h
            r = step(xp[d][:, t], b[d], h, W[d], c, kind, eh, ec)
            (h, eh), (c, ec) = r["h"], r["c"]
            gates[t] = torch.stack([r[k][0] for k in "ifgo"], -1)
            cst[t] = c
            out[:, t, d * H:(d + 1) * H], eout[:, t, d * H:(d + 1) * H] = h, eh
        res["gates"].append(gates); res["cst"].append(cst); res["hprev"].append(hprev)
        res["hn"].append((h, eh)); res["cn"].append((c, ec))
    res["out"] = (out, eout)
    return res


def seq_bwd(dout, gates, cst, c0, W, tanh="fast", cadd=2):
    """dout [B][T][2H]; gates[d] [T][B][H][4], cst[d] [T][B][H] (the stashes the kernel reads), c0[d] [B][H] or None, W[d] [4H][H]
    -> dgates[d] [B][T][4H] (gate-major) as (ref, bound), e(dc) and e(dgates) carried through the steps."""
    T, B, H = cst[0].shape
    res = []
    for d in range(2):
        Wd, G, C = D(W[d]), D(gates[d]), D(cst[d])
        dg, edg = torch.zeros(B, T, 4 * H, dtype=torch.float64), torch.zeros(B, T, 4 * H, dtype=torch.float64)
        dc, edc = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
        rec, erec = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
        for s in range(T - 1, -1, -1):
            t = s if d == 0 else T - 1 - s
            tp = t - 1 if d == 0 else t + 1
            cprev = C[tp] if s > 0 else (None if c0[d] is None else D(c0[d]))
            dh = D(dout[:, t, d * H:(d + 1) * H]) + rec
            r = cell_bwd(G[t, :, :, 0], G[t, :, :, 1], G[t, :, :, 2], G[t, :, :, 3], C[t], cprev, dc, dh, edc, U32 * dh.abs() + erec, tanh)
            dg[:, t], edg[:, t] = dgates_of(r)
            dc, edc = r["dcprev"]
            rec = dg[:, t] @ Wd
            erec = (4 * H + cadd) * U32 * (dg[:, t].abs() @ Wd.abs()) + edg[:, t] @ Wd.abs()
        res.append((dg, edg))
    return res


def bwd_step(dgn, W, dout, gst, cst, cprev, dc, cadd):
    """One step of the stage-1 backward recurrence (mmego_lstm_bwd_step): dgn [Bn][4H] the gate gradients of the step before in backward
    order (inputs), W [4H][H], gst [Bn][4H] gate-major, cst / cprev / dc [Bn][H] -> cell_bwd's dict (libm tanhf)."""
    H = W.shape[1]
    rec = D(dgn) @ D(W)
    erec = (4 * H + cadd) * U32 * (D(dgn).abs() @ D(W).abs())
    dh = D(dout) + rec
    g = D(gst)
    return cell_bwd(g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:], cst, cprev, dc, dh, 0.0, U32 * dh.abs() + erec, "libm")


# ---------------------------------------------------------------------------------------------------------------------------------
# stage-1 loss and 6-D head (imu_loss_kernel, imu_head_kernel, imu_head_bwd_kernel): running error analysis
# ---------------------------------------------------------------------------------------------------------------------------------
class EB:
    """A float64 value with a first-order fp32 error bound beside it: every operation propagates its operands' bounds through its
    partial derivatives and adds one rounding, u |result| (an fma only saves roundings).  Division and sqrtf are correctly rounded
    (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt); inputs are exact."""

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def of(x):
        return x if isinstance(x, EB) else EB(torch.as_tensor(x, dtype=torch.float64))

    def __add__(a, b):
        b = EB.of(b)
        v = a.v + b.v
        return EB(v, a.e + b.e + U32 * v.abs())

    def __sub__(a, b):
        b = EB.of(b)
        v = a.v - b.v
        return EB(v, a.e + b.e + U32 * v.abs())

    def __mul__(a, b):
        b = EB.of(b)
        v = a.v * b.v
        return EB(v, a.v.abs() * b.e + b.v.abs() * a.e + U32 * v.abs())

    def __truediv__(a, b):
        b = EB.of(b)
        v = a.v / b.v
        return EB(v, a.e / b.v.abs() + v.abs() * b.e / b.v.abs() + U32 * v.abs())

    def exact(a, k):
        """times a power of two, or a sign: no rounding"""
        return EB(a.v * k, a.e * abs(k))

    def sqrt(a):
        v = torch.sqrt(a.v)
        return EB(v, torch.where(v > 0, a.e / (2 * v).clamp_min(1e-300), torch.sqrt(a.e)) + U32 * v)

    def clamp_min(a, lo):
        return EB(a.v.clamp_min(lo), a.e)

    def where(a, m, other=0.0):
        o = EB.of(other)
        return EB(torch.where(m, a.v, o.v.expand_as(a.v)), torch.where(m, a.e, o.e.expand_as(a.e)))


def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _pairs(xs):
    return torch.stack([x.v for x in xs], -1), torch.stack([x.e + TINY for x in xs], -1)


F32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
ONE_M = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(1e-7, dtype=torch.float32))      # fl(1 - 1e-7f) = 1 - 2^-23
RAD2DEG = float(torch.tensor(180.0, dtype=torch.float32) / torch.tensor(3.14159265358, dtype=torch.float32))
ACOSF_ULP = 4.0          # OpenCL's full-profile bound for acos, which OCML is built to
EPS_HEAD = F32(1e-8)


def imu_loss(R, t, Rg, hg, scale):
    """imu_loss_kernel restated -> loss (scalar), dR [F][9], dt [F][3] as (ref, bound): sum_f acos(clamp((tr(R Rg^T) - 1) / 2)) rad2deg
    + 100 |t - head|, the gradients scaled by `scale`; rad2deg, 1e-7 and the clamp limit fl(1 - 1e-7f) = 1 - 2^-23 are the kernel's fp32
    values.  acosf: ACOSF_ULP, with the slope 1 / sqrt(1 - c^2) of the propagated part taken at the end of the error interval nearer the
    clamp (it grows without bound there).  A clamped frame contributes acos(limit) and no gradient; a frame whose cosine lies within
    its own error of the limit has no reference (asserted: the tests' inputs keep away).  The frame sum runs in double: only its final
    rounding to fp32 counts."""
    scale = F32(scale)
    a, b = [EB(R[:, k]) for k in range(9)], [EB(Rg[:, k]) for k in range(9)]
    tr = a[0] * b[0]
    for k in range(1, 9):
        tr = tr + a[k] * b[k]
    cosv = (tr - 1.0).exact(0.5)
    inside = cosv.v.abs() < ONE_M
    assert not bool((((cosv.v.abs() - ONE_M).abs() <= 2 * cosv.e) & (cosv.v.abs() != 1.0)).any()), "a cosine within its rounding error of the clamp"
    cc = EB(cosv.v.clamp(-ONE_M, ONE_M), torch.where(inside, cosv.e, torch.zeros_like(cosv.e)))
    cw = (cc.v.abs() + cc.e).clamp_max(ONE_M)
    av = torch.acos(cc.v)
    ang = EB(av, cc.e / torch.sqrt(1 - cw * cw) + ACOSF_ULP * ULP * av) * RAD2DEG
    q = EB(1.0) - cc * cc
    # (the slope of 1 / sqrt(q) likewise at the interval's end: q >= 1 - cw^2)
    sq = q.sqrt()
    sq = EB(sq.v, sq.e * torch.sqrt(q.v / (1 - cw * cw).clamp_min(1e-300)))
    g = (((EB(-RAD2DEG) / sq).exact(0.5)) * scale).where(inside)
    dR = [g * b[k] for k in range(9)]
    dv = [EB(t[:, k]) - EB(hg[:, k]) for k in range(3)]
    nrm = _dot3(dv, dv).sqrt()
    pos = nrm.v > 0
    s = ((EB(100.0) * scale) / EB(torch.where(pos, nrm.v, torch.ones_like(nrm.v)), nrm.e)).where(pos)
    dt = [s * dv[k] for k in range(3)]
    loss = ang.v.sum() + 100.0 * nrm.v.sum()
    e_loss = ang.e.sum() + 100.0 * nrm.e.sum() + U32 * loss.abs()
    return (loss, e_loss), _pairs(dR), _pairs(dt)


def imu_loss_autograd(R, t, Rg, hg, scale):
    """The same forward differentiated by float64 autograd (the check of imu_loss's restated gradients)."""
    R64, t64 = D(R).clone().requires_grad_(True), D(t).clone().requires_grad_(True)
    cc = (((R64 * D(Rg)).sum(1) - 1) * 0.5).clamp(-ONE_M, ONE_M)
    loss = (torch.acos(cc) * RAD2DEG).sum() + 100.0 * (t64 - D(hg)).norm(dim=1).sum()
    (loss * F32(scale)).backward()
    return loss.detach(), R64.grad, t64.grad


def head_fwd64(y):
    """The 6-D head restated in float64 torch (IMU_Net.py:7-18 with v / max(|v|, 1e-8)): y [F][9] -> R [F][3][3] (columns x, y, z), t."""
    a, b = y[:, 0:3], y[:, 3:6]
    x = a / a.norm(dim=1, keepdim=True).clamp_min(EPS_HEAD)
    w = torch.linalg.cross(x, b)
    z = w / w.norm(dim=1, keepdim=True).clamp_min(EPS_HEAD)
    return torch.stack((x, torch.linalg.cross(z, x), z), -1), y[:, 6:9]


def imu_head(y):
    """-> R [F][9], t [F][3] as (ref, bound): rot6d_fwd's operations through EB (the reference values are head_fwd64's)."""
    a, b = [EB(y[:, k]) for k in range(3)], [EB(y[:, 3 + k]) for k in range(3)]
    na = _dot3(a, a).sqrt().clamp_min(EPS_HEAD)
    x = [a[k] / na for k in range(3)]
    w = _cross(x, b)
    nw = _dot3(w, w).sqrt().clamp_min(EPS_HEAD)
    z = [w[k] / nw for k in range(3)]
    yy = _cross(z, x)
    Rv, Re = _pairs([c[i] for i in range(3) for c in (x, yy, z)])
    R64, t64 = head_fwd64(D(y))
    assert (R64.reshape(-1, 9) - Rv).abs().max() < 1e-9
    return (R64.reshape(-1, 9), Re), (t64, torch.zeros_like(t64))


def imu_head_bwd(y, dR, dt):
    """-> dy [F][9] as (ref, bound): the reference by float64 autograd of head_fwd64, the bound by imu_head_bwd_kernel's operations
    through EB (whose values must agree with autograd: asserted).  The kernel decides `norm > eps` on its fp32 norms; a frame whose
    norm lies within its error of eps has no reference (asserted)."""
    y64 = D(y).clone().requires_grad_(True)
    R64, t64 = head_fwd64(y64)
    ((R64.reshape(-1, 9) * D(dR)).sum() + (t64 * D(dt)).sum()).backward()
    a, b, g = [EB(y[:, k]) for k in range(3)], [EB(y[:, 3 + k]) for k in range(3)], [EB(dR[:, k]) for k in range(9)]
    na = _dot3(a, a).sqrt()
    nac = na.clamp_min(EPS_HEAD)
    x = [a[k] / nac for k in range(3)]
    w = _cross(x, b)
    nw = _dot3(w, w).sqrt()
    nwc = nw.clamp_min(EPS_HEAD)
    for n in (na, nw):
        assert not bool((((n.v - EPS_HEAD).abs() <= 2 * n.e) & (n.v != 0)).any()), "a norm within its rounding error of eps"
    z = [w[k] / nwc for k in range(3)]
    gx, gy, gz = [g[0], g[3], g[6]], [g[1], g[4], g[7]], [g[2], g[5], g[8]]
    tmp = _cross(x, gy)
    gz = [gz[k] + tmp[k] for k in range(3)]
    tmp = _cross(gy, z)
    gx = [gx[k] + tmp[k] for k in range(3)]
    big = nw.v > EPS_HEAD
    dz = _dot3(z, gz)
    gw = [((gz[k] - z[k] * dz) / nwc).where(big, gz[k] / nwc) for k in range(3)]
    tmp = _cross(b, gw)
    gx = [gx[k] + tmp[k] for k in range(3)]
    ob = _cross(gw, x)
    biga = na.v > EPS_HEAD
    dx = _dot3(x, gx)
    oa = [((gx[k] - x[k] * dx) / nac).where(biga, gx[k] / nac) for k in range(3)]
    v, e = _pairs(oa + ob + [EB(dt[:, k]) for k in range(3)])
    ref = y64.grad
    assert ((ref - v).abs() <= 1e-9 * (1 + ref.abs()) + e).all(), "the restated backward is not the autograd of the restated forward"
    return ref, e


def emu_imu_loss(R, t, Rg, hg, scale):
    f = torch.float32
    scale = torch.tensor(scale, dtype=f)
    tr = torch.zeros(R.shape[0])
    for k in range(9):
        tr = tr + R[:, k] * Rg[:, k]
    cosv = (tr - 1.0) * 0.5
    lim = torch.tensor(ONE_M, dtype=f)
    cc = torch.minimum(torch.maximum(cosv, -lim), lim)
    r2d = torch.tensor(RAD2DEG, dtype=f)
    ang = torch.acos(cc) * r2d
    g = torch.where((cosv > -lim) & (cosv < lim), (-r2d / torch.sqrt(1.0 - cc * cc)) * 0.5 * scale, torch.zeros(()))
    dv = t - hg
    nrm = torch.sqrt(dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1] + dv[:, 2] * dv[:, 2])
    s = torch.where(nrm > 0, 100.0 * scale / torch.where(nrm > 0, nrm, torch.ones(())), torch.zeros(()))
    return (ang.double().sum() + 100.0 * nrm.double().sum()).float(), g.view(-1, 1) * Rg, s.view(-1, 1) * dv


def _c32(u, v):
    return torch.stack((u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]), 1)


def _n32(v):
    return torch.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).view(-1, 1)


def emu_imu_head(y):
    a, b = y[:, 0:3], y[:, 3:6]
    x = a / _n32(a).clamp_min(EPS_HEAD)
    w = _c32(x, b)
    z = w / _n32(w).clamp_min(EPS_HEAD)
    return torch.stack((x, _c32(z, x), z), -1).reshape(-1, 9), y[:, 6:9].clone()


def emu_imu_head_bwd(y, dR, dt):
    a, b = y[:, 0:3], y[:, 3:6]
    na = _n32(a)
    nac = na.clamp_min(EPS_HEAD)
    x = a / nac
    w = _c32(x, b)
    nw = _n32(w)
    nwc = nw.clamp_min(EPS_HEAD)
    z = w / nwc
    gx, gy, gz = dR[:, 0::3], dR[:, 1::3], dR[:, 2::3]
    gz = gz + _c32(x, gy)
    gx = gx + _c32(gy, z)
    gw = torch.where(nw > EPS_HEAD, (gz - z * (z * gz).sum(1, keepdim=True)) / nwc, gz / nwc)
    gx = gx + _c32(b, gw)
    oa = torch.where(na > EPS_HEAD, (gx - x * (x * gx).sum(1, keepdim=True)) / nac, gx / nac)
    return torch.cat((oa, _c32(gw, x), dt), 1)


def rotations(g, n):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2)).unsqueeze(1)
    return (q * torch.linalg.det(q).view(-1, 1, 1)).reshape(n, 9).float()


IMU_F = (1, 6, 1023, 1025)           # 1025: past the single block's 1024 threads


def imu_loss_inputs(F):
    """Frames by f % 4: 0, 3 ordinary rotations; 1: R == R_gt, a signed permutation (the trace is exactly 3: the clamped cosine, no
    gradient); 2: t == head (norm 0, no gradient)."""
    g = gen_for(7, F)
    R = rotations(g, F)
    # R_gt = R . (a rotation by 0.2 .. 2.9 rad about a random axis): the cosine keeps away from the clamp
    ax = torch.nn.functional.normalize(torch.randn(F, 3, generator=g, dtype=torch.float64), dim=1)
    th = (0.2 + 2.7 * torch.rand(F, generator=g, dtype=torch.float64)).view(-1, 1, 1)
    K = torch.zeros(F, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    Q = torch.eye(3, dtype=torch.float64) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)
    Rg = (R.double().view(F, 3, 3) @ Q).reshape(F, 9).float()
    t, hg = torch.randn(F, 3, generator=g), torch.randn(F, 3, generator=g)
    perm = torch.tensor([[0., 1, 0, 0, 0, -1, -1, 0, 0], [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 1, 1, 0, 0, 0, 1, 0]])
    for f in range(F):
        if f % 4 == 1:
            R[f] = Rg[f] = perm[(f // 4) % 3]
        if f % 4 == 2:
            hg[f] = t[f]
    return R, t, Rg, hg


def imu_head_inputs(F):
    """Ordinary y; frame 1: a zero first vector; frame 2: parallel vectors along an axis (the cross product is exactly 0 in fp32 too):
    the <= eps branches."""
    g = gen_for(8, F)
    y = torch.randn(F, 9, generator=g)
    if F > 2:
        y[1, 0:3] = 0.0
        y[2, 0:6] = torch.tensor([0.0, 2.0, 0.0, 0.0, -3.0, 0.0])
    return y, torch.randn(F, 9, generator=g), torch.randn(F, 3, generator=g)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations of the kernels' arithmetic (torch on the CPU, every operation rounded to fp32)
# ---------------------------------------------------------------------------------------------------------------------------------
_L32 = torch.tensor(LOG2E, dtype=torch.float32)


def emu_sigmoid(x):
    return 1.0 / (1.0 + torch.exp2((-x) * _L32))


def emu_tanh(x):
    return 1.0 - 2.0 * (1.0 / (1.0 + torch.exp2((2.0 * x) * _L32)))


def emu_step(xp, b, hprev, W, cprev, kind):
    """fp32: {gates [B][4H], c, h}."""
    B, H = xp.shape[0], xp.shape[1] // 4
    xb = xp if b is None else xp + b
    if kind == "first":
        P = xb
    elif kind == "small":          # two chains over alternating k, (acc0 + acc1) + (xp + b)
        P = (hprev[:, 0::2] @ W[:, 0::2].t() + hprev[:, 1::2] @ W[:, 1::2].t()) + xb
    else:
        P = hprev @ W.t() + xb
    P = P.view(B, 4, H)
    i, f, g, o = emu_sigmoid(P[:, 0]), emu_sigmoid(P[:, 1]), emu_tanh(P[:, 2]), emu_sigmoid(P[:, 3])
    c = i * g if kind == "first" else f * cprev + i * g
    return {"gates": torch.cat((i, f, g, o), -1), "c": c, "h": o * emu_tanh(c)}


def emu_seq_fwd(xp, W, b, h0, c0):
    B, T, H = xp[0].shape[0], xp[0].shape[1], xp[0].shape[2] // 4
    out = torch.zeros(B, T, 2 * H)
    res = {"gates": [], "cst": [], "hprev": [], "hn": [], "cn": []}
    for d in range(2):
        h = torch.zeros(B, H) if h0[d] is None else h0[d].clone()
        c = torch.zeros(B, H) if c0[d] is None else c0[d].clone()
        gates, cst, hprev = torch.zeros(T, B, H, 4), torch.zeros(T, B, H), torch.zeros(B, T, H)
        for s in range(T):
            t = s if d == 0 else T - 1 - s
            hprev[:, t] = h
            r = emu_step(xp[d][:, t], b[d], h, W[d], c, "lstm64")
            h, c = r["h"], r["c"]
            gates[t] = r["gates"].view(B, 4, H).permute(0, 2, 1)
            cst[t] = c
            out[:, t, d * H:(d + 1) * H] = h
        res["gates"].append(gates); res["cst"].append(cst); res["hprev"].append(hprev); res["hn"].append(h); res["cn"].append(c)
    res["out"] = out
    return res


def emu_cell_bwd(gi, gf, gg, go, tc, cprev, dc, dh):
    dcv = dc + dh * go * (1.0 - tc * tc)
    return {"di": dcv * gg * gi * (1.0 - gi), "df": dcv * cprev * gf * (1.0 - gf), "dg": dcv * gi * (1.0 - gg * gg),
            "do": dh * tc * go * (1.0 - go), "dcprev": dcv * gf}


def emu_seq_bwd(dout, gates, cst, c0, W):
    T, B, H = cst[0].shape
    res = []
    for d in range(2):
        dg, dc, rec = torch.zeros(B, T, 4 * H), torch.zeros(B, H), torch.zeros(B, H)
        for s in range(T - 1, -1, -1):
            t = s if d == 0 else T - 1 - s
            tp = t - 1 if d == 0 else t + 1
            cprev = cst[d][tp] if s > 0 else (torch.zeros(B, H) if c0[d] is None else c0[d])
            G = gates[d][t]
            r = emu_cell_bwd(G[:, :, 0], G[:, :, 1], G[:, :, 2], G[:, :, 3], emu_tanh(cst[d][t]), cprev, dc, dout[:, t, d * H:(d + 1) * H] + rec)
            dg[:, t] = torch.cat([r[k] for k in ("di", "df", "dg", "do")], -1)
            dc = r["dcprev"]
            rec = dg[:, t] @ W[d]
        res.append(dg)
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch mirrors
# ---------------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def step_kernel(first, aligned, ndir, Bn, H, ncu):
    """mmego_lstm_step's choice.  aligned: b_hh, the stashes and direction 1's xproj / hout / c all on 16-byte addresses."""
    if first and H % 4 == 0 and aligned:
        return "lstm_first_step_kernel"
    if Bn >= 128:
        grid32 = ndir * (H // 32) * cdiv(Bn, 64)
        return "lstm_step_dma_kernel<16>" if 2 * grid32 <= (ncu if ncu > 0 else 256) else "lstm_step_dma_kernel<32>"
    full = "true" if Bn % 64 == 0 else "false"
    if H == 512 and Bn % 64 == 0:
        return "lstm_step_small_kernel<64, true, 8>"
    return "lstm_step_small_kernel<%d, %s>" % (64 if H % 64 == 0 else 32, full)


def step_dma(first, ndir, Bn, H, ht):
    """-> (chunks in the 3-stage ring, barriers every wave executes, XCD order taken) of lstm_step_dma_kernel<ht>."""
    nk = 0 if first else H // 32
    return nk, (nk + 1 if nk > 0 else 2), (ndir * (H // ht)) % 8 == 0


def smallest_dma32_bn(ndir, H, ncu):
    """The smallest Bn = 64 n + 8 (ragged last row block) at which the step takes lstm_step_dma_kernel<32>."""
    n = 2
    while step_kernel(False, True, ndir, 64 * n + 8, H, ncu) != "lstm_step_dma_kernel<32>":
        n += 1
    return 64 * n + 8


def bwd_step_kernel(env, Bn, H, dgs, aligned=True):
    """lstm_bwd_step_dma_try's choice behind mmego_lstm_bwd_step's checks.  env: MMEGO_LSTM_BWD_DMA (None: unset)."""
    on = 1 if env is None else int(env)
    if (not on) or Bn % 64 != 0 or H % 32 != 0 or dgs % 4 != 0 or not aligned:
        return "gemm32kq_kernel<true, true>"
    return "lstm_bwd_step_dma_kernel"


def l64_inst(B, stash, drop):
    return "lstm64_fwd_kernel<%s, %s, %s>" % tuple("true" if v else "false" for v in (B % 16 == 0, stash, drop))


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and cases shared by the GPU file and the CPU emulation test
# ---------------------------------------------------------------------------------------------------------------------------------
def gen_for(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


def row_kinds(B, shift=0):
    """Per row: 0 / 3 ordinary, 1 saturated (pre-activations +-20 and +-100), 2 near zero (pre-activations and c below 1e-3)."""
    return (torch.arange(B) + shift) % 4


def init_w(g, H):
    """nn.LSTM's initialisation: uniform(-1 / sqrt(H), 1 / sqrt(H))."""
    k = 1.0 / math.sqrt(H)
    return (torch.rand(4 * H, H, generator=g) * 2 - 1) * k, (torch.rand(4 * H, generator=g) * 2 - 1) * k


def shape_pre(g, xp, b, kinds):
    """xp [B][..][4H] of order 1 -> saturated rows at +-20 / +-100 and near-zero rows at -b + 3e-4 randn."""
    sat = torch.where(torch.rand(xp.shape, generator=g) < 0.5, 20.0, 100.0) * torch.where(torch.rand(xp.shape, generator=g) < 0.5, -1.0, 1.0)
    small = torch.randn(xp.shape, generator=g) * 3e-4 - (0.0 if b is None else b)
    k = kinds.view(-1, *([1] * (xp.dim() - 1)))
    return torch.where(k == 1, sat, torch.where(k == 2, small, xp))


def shape_state(g, v, kinds, scale=3e-4):
    """h0 / c0 / hprev / c [B][H]: near-zero rows get values below 1e-3."""
    return torch.where(kinds.view(-1, 1) == 2, torch.randn(v.shape, generator=g).clamp(-3, 3) * scale, v)


def seq_inputs(B, T, shift=0, H=64, with_b=True):
    """The H = 64 pair's inputs: W, b [2] (None without b_hh), xp[d] [B][T][4H], h0, c0 [2][B][H], dout [B][T][2H]."""
    g = gen_for(64, B, T, shift, H)
    kinds = row_kinds(B, shift)
    W, b, xp, h0, c0 = [], [], [], [], []
    for d in range(2):
        w_, b_ = init_w(g, H)
        b_ = b_ if with_b else None
        W.append(w_); b.append(b_)
        xp.append(shape_pre(g, torch.randn(B, T, 4 * H, generator=g), b_, kinds))
        h0.append(shape_state(g, torch.randn(B, H, generator=g) * 0.5, kinds))
        c0.append(shape_state(g, torch.randn(B, H, generator=g) * 0.5, kinds))
    return {"W": W, "b": b, "xp": xp, "h0": h0, "c0": c0, "dout": torch.randn(B, T, 2 * H, generator=g), "kinds": kinds}


def step_inputs(ndir, Bn, H, key=0):
    g = gen_for(1, ndir, Bn, H, key)
    kinds = row_kinds(Bn)
    r = {"W": [], "b": [], "xp": [], "h": [], "c": [], "kinds": kinds}
    for d in range(ndir):
        w_, b_ = init_w(g, H)
        r["W"].append(w_); r["b"].append(b_)
        r["xp"].append(shape_pre(g, torch.randn(Bn, 4 * H, generator=g), b_, kinds))
        r["h"].append(shape_state(g, torch.randn(Bn, H, generator=g) * 0.5, kinds))
        r["c"].append(shape_state(g, torch.randn(Bn, H, generator=g) * 0.5, kinds))
    return r


def bwd_inputs(ndir, Bn, H, key=0):
    """Stage-1 backward inputs: stashes of a reference step rounded to fp32 (saturated and near-zero rows included), dout, dhrec, dc,
    and for the recurrent form the previous step's gate gradients dgn [Bn][4H] and W."""
    s = step_inputs(ndir, Bn, H, 100 + key)
    g = gen_for(2, ndir, Bn, H, key)
    r = {"gst": [], "cst": [], "cprev": s["c"], "W": s["W"], "dout": [], "dhrec": [], "dc": [], "dgn": [], "kinds": s["kinds"]}
    for d in range(ndir):
        st = step(s["xp"][d], s["b"][d], s["h"][d], s["W"][d], s["c"][d], "dma")
        r["gst"].append(st["gates"][0].float()); r["cst"].append(st["c"][0].float())
        r["dout"].append(torch.randn(Bn, H, generator=g)); r["dhrec"].append(torch.randn(Bn, H, generator=g) * 0.3)
        r["dc"].append(torch.randn(Bn, H, generator=g) * 0.5); r["dgn"].append(torch.randn(Bn, 4 * H, generator=g) * 0.2)
    return r


# the cases of tests/test_lstm_kernels_gpu.py (test_lstm_ref_cpu.py runs the emulation over the same ones)
L64_B = (1, 13, 16, 17, 33)
L64_T = (1, 2, 5)
# h0 and c0 given per direction, b_hh given, xs, os, then the backward's: c0 given per direction, dos, dgs
L64_OPTS = [dict(h0=(1, 1), c0=(1, 1), bhh=1, xs=512, os=128, bc0=(1, 1), dos=128, dgs=512),
            dict(h0=(0, 1), c0=(1, 0), bhh=0, xs=516, os=256, bc0=(0, 1), dos=256, dgs=516),
            dict(h0=(1, 0), c0=(0, 1), bhh=1, xs=516, os=128, bc0=(1, 0), dos=256, dgs=512),
            dict(h0=(0, 0), c0=(0, 0), bhh=1, xs=512, os=256, bc0=(0, 0), dos=128, dgs=516)]


def l64_opts(B, T, shift=0):
    """The options of the (B, T) case; B = 1 runs once per row kind (shift) with the options of that index."""
    return L64_OPTS[shift] if shift else L64_OPTS[(L64_B.index(B) * len(L64_T) + L64_T.index(T)) % len(L64_OPTS)]
# (ndir, Bn, H, first, b_hh one float past an aligned address) -> the kernel it must reach; the <32> case is added from the CU count
STEP_CASES = [
    (2, 64, 128, 1, 0, "lstm_first_step_kernel"),
    (1, 37, 96, 1, 0, "lstm_first_step_kernel"),
    (2, 64, 128, 1, 1, "lstm_step_small_kernel<64, true>"),
    (2, 37, 96, 1, 1, "lstm_step_small_kernel<32, false>"),
    (2, 136, 64, 1, 1, "lstm_step_dma_kernel<16>"),
    (2, 64, 512, 0, 0, "lstm_step_small_kernel<64, true, 8>"),
    (2, 64, 128, 0, 0, "lstm_step_small_kernel<64, true>"),
    (1, 37, 128, 0, 0, "lstm_step_small_kernel<64, false>"),
    (1, 64, 96, 0, 0, "lstm_step_small_kernel<32, true>"),
    (2, 37, 96, 0, 0, "lstm_step_small_kernel<32, false>"),
] + [(nd, Bn, H, 0, 0, "lstm_step_dma_kernel<16>") for H, nd in ((32, 2), (64, 2), (96, 1), (128, 2)) for Bn in (128, 136)]
CELL_BWD_CASES = [(nd, Bn, H) for nd in (1, 2) for Bn in (1, 37, 64) for H in (32, 96)]
# (Bn, H, MMEGO_LSTM_BWD_DMA) -> kernel
BWD_STEP_CASES = [(Bn, H, None, "lstm_bwd_step_dma_kernel") for Bn in (64, 128) for H in (32, 64, 96, 128)] + [
    (64, 512, None, "lstm_bwd_step_dma_kernel"), (32, 64, None, "gemm32kq_kernel<true, true>"), (96, 32, None, "gemm32kq_kernel<true, true>"),
    (64, 64, "0", "gemm32kq_kernel<true, true>")]


def worst_ratio(out, ref, bound):
    """Largest |out - ref| / bound over every element (bound 0: equal or inf; NaN: inf) and its index."""
    out, ref = out.double(), ref.double()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    err = (out - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
    if ratio.numel() == 0:
        return 0.0, ()
    i = int(ratio.argmax())
    return float(ratio.max()), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
