"""Float64 reference, a-priori error bound, dispatch restatement and case table of the fp32 GEMM entry points mmego_gemm and
mmego_gemm_group (csrc/gemm.hip, csrc/gemm_tile.hip; contract: include/mmego_hip.h).

The contract, on flat storage and element strides (A(m,k) = A[b*sAb + m*sam + k*sak] and so on):

    C[b](m,n) = cmulop( acc( relu1( sum_k A[b](m,k) B[b](k,n) + bias[b*sBiasb + n] ) ) )

relu1: max(., 0) for relu == 1 only; acc: + the old C for accumulate == 1 only; cmulop: * cmul for relu 0 / 1, 0 where cmul <= 0 for
relu == 2; asum[b*M + m] (+)= sum_k A[b](m,k) following accumulate.  accumulate == 2 (deferred split-K): C is not touched, the
nsplit slabs [nsplit][nbatch*M*N] at the front of splitk_ws add up to the product, and with asum the slab row sums
[nsplit][nbatch*M] sit behind them.

ref() restates this in float64, bound() is the path-independent bound of an fp32 evaluation in ANY summation order:

    |out - ref| <= (K + 4) u (sum_k |a||b| + |bias| + |C0|) max(1, |cmul|),     u = 2^-24

Any order of summing K fp32 products passes each term through at most K roundings (one for the product, at most K - 1 additions on
its way to the root of whatever tree: the four quarters of the small-tile kernel, the K slabs, the reducer's 16 lanes), which gives
(1 + u)^K - 1 <= K u (1 + second order) per term; the + 4 pays for the zero seed of the accumulator, the bias, the old C and the
multiplier, each one more rounding of everything before it.  ReLU and the mask do not round and are 1-Lipschitz.  The callers
multiply by 1.001 for the second-order term (K u <= 2^-12 here); there is no other margin and nothing measured in it.

Two data sets per case.  "int": A, B, bias, C0 integers in [-7, 7], cmul in {-1, 0, 1, 2}: every partial sum in every order is an
integer of magnitude <= 49 K + 14 < 2^24, so every kernel must return the float64 result EXACTLY -- the set that catches index, edge,
clamp and slab mistakes.  "normal": unit-normal values against bound() -- the set that catches an operand of reduced precision (an
operand rounded to bf16 errs by about 2^-9 sqrt(K) 0.6 per output: far outside the bound at K <= 192).

Every buffer is larger than the contract needs.  Outputs (C, asum, splitk_ws) are pre-filled with one NaN bit pattern, compared as
int32, that has to survive wherever the contract does not write: between strided rows and columns, past M and N, between batch
entries, behind the documented workspace size, and in all of C under accumulate == 2.  Inputs have NaN around and between their
elements, so a clamped or stray read that reaches a sum shows in the result.
"""
import math

import torch

from mmego_amd import ops

U = 2.0 ** -24
SECOND_ORDER = 1.001
SENTINEL = 0x7FC5A5A5            # a quiet NaN with a payload nothing computes
GUARD = 64                       # floats in front of and behind every buffer (a multiple of 4: alignment is the case's choice)
GROUP_MAX = 10                   # csrc/gemm.hip GEMM_GROUP_MAX (mmego_gemm_group's documented limit)

LABELS = ("g64_bk16", "g64_bk64", "kq", "g128nt", "tile64", "tile128", "persist_halves", "persist_whole", "big", "big_slabs")
# the persistent walk is taken from K > 128 only (gemm_tile.hip: two chunks per tile run on the plain grid) and K is a multiple of 64
# on the tile paths: 192 is the shortest K that reaches it
PERSIST_MIN_K = 192


def cdiv(a, b):
    return -(-a // b)


class Case:
    """One mmego_gemm argument set.  orient: first letter A, second B; A 'N' = A[m][k] (k contiguous), 'T' = A[k][m];
    B 'N' = B[k][n] (n contiguous), 'T' = B[n][k] (k contiguous) -- "NT" is the Linear form, both operands k-contiguous.
    scn: column stride of a row-major C; ccol: column-major C (scm == 1); gap: floats between batch entries; misalign: both operands
    start one float behind a 16-byte boundary; bias_b: one bias per batch entry (sBiasb != 0); pair: the batch entries share ONE A
    (sAb == 0) and write column blocks of ONE row-major C (sCb == N: ops.linear_pair's form, the two directions' input projections
    of a BiLSTM layer).  override: ABI values replaced after the buffers are built (the refusals: M = 0, a null pointer, ...)."""

    def __init__(self, name, label, M, N, K, orient="NN", nbatch=1, nsplit=1, relu=0, accumulate=0, bias=False, bias_b=False,
                 cmul=False, asum=False, scn=1, ccol=False, gap=False, misalign=False, pair=False, override=None):
        self.name, self.label = name, label
        self.M, self.N, self.K, self.orient = M, N, K, orient
        self.nbatch, self.nsplit, self.relu, self.accumulate = nbatch, nsplit, relu, accumulate
        self.bias, self.bias_b, self.cmul, self.asum = bias or bias_b, bias_b, cmul, asum
        self.scn, self.ccol, self.gap, self.misalign, self.pair = scn, ccol, gap, misalign, pair
        assert not (pair and (ccol or gap or scn != 1))
        self.override = dict(override or {})

    def __repr__(self):
        return "Case(%s)" % self.name

    @property
    def options(self):
        """The option names of the issue's list this case carries."""
        o = set()
        if self.cmul and self.relu != 2:
            o.add("cmul")
            if self.nbatch > 1:
                o.add("cmul_nbatch")
        if self.relu == 2:
            o.add("cmask")
        if self.asum:
            o.add("asum")
            if self.accumulate == 1:
                o.add("asum_accumulate")
            if self.nsplit > 1:
                o.add("asum_nsplit")
            if self.accumulate == 2:
                o.add("asum_deferred")
        if self.scn != 1:
            o.add("strided_c")
        if self.relu == 1 and self.accumulate == 1 and self.bias:
            o.add("relu_accumulate_bias")
        return o


class Layout:
    """Element strides, offsets into the flat buffers and buffer lengths of a case."""

    def __init__(self, c):
        M, N, K, nb = c.M, c.N, c.K, c.nbatch
        up4 = lambda v: cdiv(v, 4) * 4
        a_kc, b_kc = c.orient[0] == "N", c.orient[1] == "T"
        # operands: leading dimension = the contiguous extent rounded up to 4, plus 4 floats of NaN; batch entries a further 8 apart
        self.lda = up4(K if a_kc else M) + 4
        self.ldb = up4(K if b_kc else N) + 4
        self.sam, self.sak = (self.lda, 1) if a_kc else (1, self.lda)
        self.sbn, self.sbk = (self.ldb, 1) if b_kc else (1, self.ldb)
        self.sAb = 0 if c.pair else (M if a_kc else K) * self.lda + (8 if c.gap else 0)
        self.sBb = (N if b_kc else K) * self.ldb + (8 if c.gap else 0)
        self.offA = self.offB = GUARD + (1 if c.misalign else 0)
        self.lenA = self.offA + (nb * self.sAb if self.sAb else (M if a_kc else K) * self.lda) + GUARD
        self.lenB = self.offB + nb * self.sBb + GUARD
        # C: row-major with column stride scn and 3 more floats per row, or column-major with 3 more floats per column
        if c.pair:
            self.scm, self.scn, self.sCb = nb * N + 3, 1, N
        elif c.ccol:
            self.scm, self.scn = 1, M + 3
            self.sCb = N * self.scn + (12 if c.gap else 0)
        else:
            self.scn = c.scn
            self.scm = N * c.scn + 3
            self.sCb = M * self.scm + (12 if c.gap else 0)
        self.offC = GUARD
        self.lenC = self.offC + (M * self.scm if c.pair else nb * self.sCb) + GUARD
        self.sBiasb = N + 5 if c.bias_b else 0
        self.lenBias = GUARD + nb * (N + 5) + GUARD
        self.lenAsum = GUARD + nb * M + GUARD
        self.ws_need = ws_floats(M, N, nb, c.nsplit, c.asum)
        self.lenWs = self.ws_need + GUARD


def ws_floats(M, N, nbatch, nsplit, asum):
    """The documented size of splitk_ws: nsplit*nbatch*M*N floats, and nsplit*nbatch*M more with asum."""
    return nsplit * nbatch * M * N + (nsplit * nbatch * M if asum else 0)


def views(c, bufs):
    """The contract's index maps as strided views of the flat buffers: A [nb][M][K], B [nb][K][N], C / cmul [nb][M][N],
    bias [nb][N], asum [nb][M]."""
    L, nb = Layout(c), c.nbatch
    st = lambda buf, off, size, stride: torch.as_strided(buf, size, stride, off)
    v = {"A": st(bufs["A"], L.offA, (nb, c.M, c.K), (L.sAb, L.sam, L.sak)),
         "B": st(bufs["B"], L.offB, (nb, c.K, c.N), (L.sBb, L.sbk, L.sbn)),
         "C": st(bufs["C"], L.offC, (nb, c.M, c.N), (L.sCb, L.scm, L.scn))}
    if c.bias:
        v["bias"] = st(bufs["bias"], GUARD, (nb, c.N), (L.sBiasb, 1))
    if c.cmul:
        v["cmul"] = st(bufs["cmul"], L.offC, (nb, c.M, c.N), (L.sCb, L.scm, L.scn))
    if c.asum:
        v["asum"] = st(bufs["asum"], GUARD, (nb, c.M), (c.M, 1))
    return v


def _sentinel(n, device):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)


def make_bufs(c, kind, device="cpu", seed=0):
    """Flat fp32 buffers of a case, filled for data set `kind` ("int" or "normal").  Inputs: NaN wherever the contract does not read.
    Outputs: the sentinel wherever the contract does not write -- and where it writes without reading (C and asum without accumulate),
    so that an element the kernel leaves out shows as well."""
    L = Layout(c)
    g = torch.Generator(device=device).manual_seed(1000003 * seed + sum(map(ord, c.name)) + (7 if kind == "int" else 0))

    def draw(shape):
        if kind == "int":
            return torch.randint(-7, 8, shape, generator=g, device=device).float()
        return torch.randn(shape, generator=g, device=device)

    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=device)
    bufs = {"A": nan(L.lenA), "B": nan(L.lenB), "C": _sentinel(L.lenC, device), "bias": None, "cmul": None, "asum": None, "ws": None}
    if c.bias:
        bufs["bias"] = nan(L.lenBias)
    if c.cmul:
        bufs["cmul"] = nan(L.lenC)
    if c.asum:
        bufs["asum"] = _sentinel(L.lenAsum, device)
    if c.nsplit > 1:
        bufs["ws"] = _sentinel(L.lenWs, device)
    v = views(c, bufs)
    if c.pair:
        v["A"][0].copy_(draw(v["A"].shape[1:]))
    else:
        v["A"].copy_(draw(v["A"].shape))
    v["B"].copy_(draw(v["B"].shape))
    if c.bias:
        if c.bias_b:
            v["bias"].copy_(draw(v["bias"].shape))
        else:
            v["bias"][0].copy_(draw((c.N,)))
    if c.accumulate:
        v["C"].copy_(draw(v["C"].shape))
        if c.asum and c.accumulate == 1:
            v["asum"].copy_(draw(v["asum"].shape))
    if c.cmul:
        shape = v["cmul"].shape
        if kind == "int":
            m = torch.randint(-1, 3, shape, generator=g, device=device).float()
        else:                                            # a quarter exact zeros: the mask's boundary (cmul <= 0)
            m = torch.randn(shape, generator=g, device=device)
            m = torch.where(torch.rand(shape, generator=g, device=device) < 0.25, torch.zeros_like(m), m)
        v["cmul"].copy_(m)
    return bufs


def ref(c, bufs):
    """float64 restatement of the contract from the buffers as they are BEFORE the call.  -> {"C": [nb][M][N] or None (deferred),
    "prod": the plain product (what the deferred slabs add up to), "asum": [nb][M] or None}."""
    v = views(c, bufs)
    A, B = v["A"].double(), v["B"].double()
    prod = torch.matmul(A, B)
    out = {"prod": prod, "C": None, "asum": None}
    if c.asum:
        rows = A.sum(2)
        out["asum"] = rows + v["asum"].double() if c.accumulate == 1 else rows
    if c.accumulate == 2:
        return out
    x = prod
    if c.bias:
        x = x + v["bias"].double()[:, None, :]
    if c.relu == 1:
        x = x.clamp_min(0.0)
    if c.accumulate == 1:
        x = x + v["C"].double()
    if c.cmul:
        cm = v["cmul"].double()
        x = torch.where(cm > 0, x, torch.zeros_like(x)) if c.relu == 2 else x * cm
    out["C"] = x
    return out


def bound(c, bufs):
    """The a-priori bound of the module docstring, same keys as ref() (without the 1.001)."""
    v = views(c, bufs)
    A, B = v["A"].double().abs(), v["B"].double().abs()
    t = torch.matmul(A, B)
    f = (c.K + 4) * U
    out = {"prod": f * t, "C": None, "asum": None}
    if c.asum:
        rows = A.sum(2)
        out["asum"] = f * (rows + v["asum"].double().abs() if c.accumulate == 1 else rows)
    if c.accumulate == 2:
        return out
    if c.bias:
        t = t + v["bias"].double().abs()[:, None, :]
    if c.accumulate == 1:
        t = t + v["C"].double().abs()
    t = f * t
    if c.cmul and c.relu != 2:
        t = t * v["cmul"].double().abs().clamp_min(1.0)
    out["C"] = t
    return out


def fp32_eval(c, bufs):
    """The contract evaluated in fp32 (torch.matmul and the epilogue in fp32): what bound() has to contain.  Same keys as ref()."""
    v = views(c, bufs)
    prod = torch.matmul(v["A"], v["B"])
    out = {"prod": prod, "C": None, "asum": None}
    if c.asum:
        rows = v["A"].sum(2)
        out["asum"] = rows + v["asum"] if c.accumulate == 1 else rows
    if c.accumulate == 2:
        return out
    x = prod
    if c.bias:
        x = x + v["bias"][:, None, :]
    if c.relu == 1:
        x = x.clamp_min(0.0)
    if c.accumulate == 1:
        x = x + v["C"]
    if c.cmul:
        x = torch.where(v["cmul"] > 0, x, torch.zeros_like(x)) if c.relu == 2 else x * v["cmul"]
    out["C"] = x
    return out


def written_mask(c, bufs):
    """int32 copies' helper: {buffer name: bool mask of the floats the contract lets the call write}."""
    L, nb = Layout(c), c.nbatch
    m = {}
    mc = torch.zeros(L.lenC, dtype=torch.bool, device=bufs["C"].device)
    if c.accumulate != 2:
        torch.as_strided(mc, (nb, c.M, c.N), (L.sCb, L.scm, L.scn), L.offC).fill_(True)
    m["C"] = mc
    if c.asum:
        ma = torch.zeros(L.lenAsum, dtype=torch.bool, device=mc.device)
        if c.accumulate != 2:
            ma[GUARD:GUARD + nb * c.M] = True
        m["asum"] = ma
    if c.nsplit > 1:
        mw = torch.zeros(L.lenWs, dtype=torch.bool, device=mc.device)
        mw[:L.ws_need] = True
        m["ws"] = mw
    return m


def abi(c, bufs=None):
    """mmego_gemm's arguments behind the stream, by name, in the header's order.  With bufs: pointers are tensor views (or None);
    without: 16-byte alignment of the operand pointers as booleans under A / B and presence as booleans elsewhere -- what path_of
    reads."""
    L = Layout(c)
    if bufs is None:
        p = lambda name, off=0: True
        A, B = not c.misalign, not c.misalign
    else:
        p = lambda name, off=0: bufs[name][off:]
        A, B = p("A", L.offA), p("B", L.offB)
    a = {"A": A, "sam": L.sam, "sak": L.sak, "B": B, "sbk": L.sbk, "sbn": L.sbn, "C": p("C", L.offC), "scm": L.scm, "scn": L.scn,
         "bias": p("bias", GUARD) if c.bias else None, "M": c.M, "N": c.N, "K": c.K, "nbatch": c.nbatch,
         "sAb": L.sAb, "sBb": L.sBb, "sCb": L.sCb, "relu": c.relu, "accumulate": c.accumulate,
         "splitk_ws": p("ws") if c.nsplit > 1 else None, "nsplit": c.nsplit, "sBiasb": L.sBiasb,
         "cmul": p("cmul", L.offC) if c.cmul else None, "asum": p("asum", GUARD) if c.asum else None}
    a.update(c.override)
    return a


def _general_path(a):
    """The strided kernels' choice (gemm.hip behind the tile and fast branches) -> (label or None when refused, kchunk)."""
    kchunk = cdiv(cdiv(a["K"], a["nsplit"]), 16) * 16
    wgs64 = cdiv(a["M"], 64) * cdiv(a["N"], 64) * a["nbatch"] * a["nsplit"]
    if wgs64 <= ops._KQ_MAX and kchunk >= 64:
        return "kq", kchunk
    return ("g64_bk64" if kchunk >= 64 else "g64_bk16"), kchunk


def path_of(c):
    """The launcher's dispatch (mmego_gemm of csrc/gemm.hip, gemm_tile_launch of csrc/gemm_tile.hip) restated: the kernel a case
    runs on, "+reduce" when splitk_reduce follows, "refused" when the launcher returns bad-argument."""
    a = abi(c)
    M, N, K, nb, ns = a["M"], a["N"], a["K"], a["nbatch"], a["nsplit"]
    relu, acc = a["relu"], a["accumulate"]
    if not (a["A"] is not None and a["B"] is not None and a["C"] is not None and M > 0 and N > 0 and K > 0 and nb > 0 and ns >= 1):
        return "refused"
    defer = acc == 2
    if defer and not (ns > 1 and nb == 1 and a["bias"] is None and not relu):
        return "refused"
    if a["cmul"] is not None and ns != 1:
        return "refused"
    if not (relu in (0, 1) or (relu == 2 and a["cmul"] is not None)):
        return "refused"
    if a["sBiasb"] != 0 and ns != 1:
        return "refused"
    reduce_ = "+reduce" if ns > 1 and not defer else ""
    aligned = a["A"] is True and a["B"] is True
    a_kc, b_kc = a["sak"] == 1, a["sbk"] == 1
    a_mc, b_mc = a["sam"] == 1 and not a_kc, a["sbn"] == 1 and not b_kc
    lda, ldw = (a["sam"] if a_kc else a["sak"]), (a["sbn"] if b_kc else a["sbk"])
    kchunk_t = cdiv(cdiv(K, ns), 64) * 64 if ns > 1 else K
    tile_min = (1 if K <= 1024 else 200) if (a_kc and b_kc and ns == 1) else ops._TILE_MIN_OTHER
    units64 = (M // 64) * (N // 64) * ns * nb
    tile = (a["cmul"] is None and a["asum"] is None and a["scn"] == 1 and (nb == 1 or (a["sAb"] % 4 == 0 and a["sBb"] % 4 == 0))
            and (a_kc or a_mc) and (b_kc or b_mc) and lda % 4 == 0 and ldw % 4 == 0 and aligned and M % 64 == 0 and N % 64 == 0
            and K % 64 == 0 and units64 >= tile_min and (ns == 1 or (ns - 1) * kchunk_t < K))
    if tile and not (ns > 1 and a["splitk_ws"] is None):
        if a_kc and b_kc:
            tiles = (M // 320) * (N // 256) * nb
            slab_ok = (not acc) if ns == 1 else (acc == 2 and nb == 1 and a["bias"] is None and kchunk_t >= 64 and
                                                 (ns - 1) * kchunk_t < K and K - (ns - 1) * kchunk_t >= 64)
            units = tiles * ns
            if M % 320 == 0 and N % 256 == 0 and K >= 64 and slab_ok and not relu and units >= 256 and units % 256 == 0:
                return "big" if ns == 1 else "big_slabs"
        units128 = (M // 128) * (N // 128) * ns * nb
        if M % 128 == 0 and N % 128 == 0 and units128 >= 192:
            if units128 > 512 and K > 128:
                rest = units128 % 512
                return ("persist_halves" if 0 < rest <= 256 else "persist_whole") + reduce_
            return "tile128" + reduce_
        return "tile64" + reduce_
    if (a["cmul"] is None and a["asum"] is None and nb == 1 and ns == 1 and not acc and a_kc and b_kc and a["scn"] == 1
            and M % 128 == 0 and N % 128 == 0 and K % 16 == 0 and a["sam"] % 4 == 0 and a["sbn"] % 4 == 0 and aligned):
        return "g128nt"
    if ns > 1 and a["splitk_ws"] is None:
        return "refused"
    if cdiv(N, 32) > 65535 or nb * ns > 65535:
        return "refused"
    label, _ = _general_path(a)
    if a["asum"] is not None and label != "kq":
        return "refused"
    return label + reduce_


def group_path_of(cases):
    """mmego_gemm_group: "group" when the entries share one launch of the K-quartered kernel, "fallback" when they run as separate
    mmego_gemm calls, "refused" when an entry is one mmego_gemm refuses."""
    n = len(cases)
    if n < 1 or any(path_of(c) == "refused" for c in cases):
        return "refused"
    if not 2 <= n <= GROUP_MAX:
        return "fallback"
    a0 = abi(cases[0])
    akc, bkc = a0["sak"] == 1, a0["sbk"] == 1
    z = 0
    for c in cases:
        a = abi(c)
        units64 = (a["M"] // 64) * (a["N"] // 64) * a["nbatch"]
        wgs64 = cdiv(a["M"], 64) * cdiv(a["N"], 64) * a["nbatch"]
        if not (a["nsplit"] == 1 and (a["sak"] == 1) == akc and (a["sbk"] == 1) == bkc and not (akc and bkc)
                and units64 < ops._TILE_MIN_OTHER and wgs64 <= ops._KQ_MAX and a["K"] >= 64 and a["relu"] != 2
                and cdiv(a["N"], 32) <= 65535):
            return "fallback"
        z += a["nbatch"]
    return "group" if z <= 65535 else "fallback"


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table: the smallest shapes that reach each path
# ---------------------------------------------------------------------------------------------------------------------------------
def _cases():
    C, t = Case, []
    # gemm64<BK=16>: a K range per workgroup below 64
    t += [C("g16_1x1x1", "g64_bk16", 1, 1, 1),
          C("g16_70x33x17_bias_relu_acc", "g64_bk16", 70, 33, 17, "NN", bias=True, relu=1, accumulate=1),
          C("g16_65x65x47_tt_scn2", "g64_bk16", 65, 65, 47, "TT", scn=2),
          C("g16_70x33x17_nt_ccol", "g64_bk16", 70, 33, 17, "NT", ccol=True, bias=True),
          C("g16_split3_chunk48", "g64_bk16+reduce", 70, 33, 100, "NT", nsplit=3, bias=True),
          C("g16_split4_empty_slab", "g64_bk16+reduce", 40, 40, 33, "TN", nsplit=4, bias=True, relu=1, accumulate=1),
          C("g16_split4_deferred", "g64_bk16", 40, 40, 33, "NN", nsplit=4, accumulate=2),
          C("g16_cmul_misaligned", "g64_bk16", 70, 33, 17, "NT", cmul=True, misalign=True),
          C("g16_cmask_bias_acc", "g64_bk16", 65, 65, 47, "NN", cmul=True, relu=2, bias=True, accumulate=1),
          C("g16_cmul_nbatch2", "g64_bk16", 70, 33, 17, "TN", cmul=True, nbatch=2, gap=True, relu=1, bias_b=True)]
    # gemm32kq: at most GEMM_KQ_MAX 64x64 workgroups and a K range of at least 64
    t += [C("kq_70x33x100_nn", "kq", 70, 33, 100, "NN"),
          C("kq_70x33x100_nt_bias_relu_acc", "kq", 70, 33, 100, "NT", bias=True, relu=1, accumulate=1),
          C("kq_70x33x100_tn_ccol", "kq", 70, 33, 100, "TN", ccol=True, bias=True),
          C("kq_70x33x100_tt_scn3", "kq", 70, 33, 100, "TT", scn=3, relu=1)]
    for K in (64, 65, 127, 128, 129, 200):               # uneven quarters; vector loads with scalar tails (NT), scalar loads (TN)
        t += [C("kq_37x35x%d_nt" % K, "kq", 37, 35, K, "NT", bias=True), C("kq_37x35x%d_tn" % K, "kq", 37, 35, K, "TN", accumulate=1)]
    t += [C("kq_m1", "kq", 1, 40, 64, "NN", bias=True), C("kq_n1", "kq", 40, 1, 64, "TT"), C("kq_1x1x64", "kq", 1, 1, 64, "NT"),
          C("kq_33x31x64", "kq", 33, 31, 64, "NN", relu=1),
          C("kq_split4", "kq+reduce", 70, 33, 300, "TN", nsplit=4, bias=True, relu=1, accumulate=1),
          C("kq_split5_empty_slab", "kq+reduce", 40, 40, 250, "NT", nsplit=5),
          C("kq_split4_deferred", "kq", 70, 33, 300, "TN", nsplit=4, accumulate=2),
          C("kq_nbatch3_gap", "kq", 70, 33, 100, "NN", nbatch=3, gap=True, bias_b=True, relu=1, accumulate=1),
          C("kq_nbatch3_gap_tt_ccol", "kq", 70, 33, 100, "TT", nbatch=3, gap=True, ccol=True),
          C("kq_pair", "kq", 70, 33, 100, "NT", nbatch=2, pair=True, bias_b=True),
          C("kq_misaligned_nt", "kq", 70, 33, 129, "NT", misalign=True, bias=True),
          C("kq_misaligned_tn", "kq", 70, 33, 129, "TN", misalign=True),
          C("kq_cmul", "kq", 70, 33, 100, "NN", cmul=True, bias=True, relu=1, accumulate=1),
          C("kq_cmul_scn2", "kq", 37, 35, 65, "NT", cmul=True, scn=2),
          C("kq_cmask", "kq", 70, 33, 100, "NT", cmul=True, relu=2),
          C("kq_cmask_bias_acc", "kq", 70, 33, 100, "TN", cmul=True, relu=2, bias=True, accumulate=1),
          C("kq_cmul_nbatch2", "kq", 70, 33, 100, "NN", cmul=True, nbatch=2, gap=True),
          C("kq_asum_n100", "kq", 40, 100, 100, "TN", asum=True),
          C("kq_asum_n100_nt", "kq", 45, 100, 127, "NT", asum=True, bias=True),
          C("kq_asum_accumulate", "kq", 40, 100, 100, "TN", asum=True, accumulate=1),
          C("kq_asum_nbatch2", "kq", 40, 100, 64, "TN", asum=True, nbatch=2, gap=True),
          C("kq_asum_split3", "kq+reduce", 40, 100, 300, "TN", asum=True, nsplit=3),
          C("kq_asum_split3_accumulate", "kq+reduce", 40, 100, 300, "TN", asum=True, nsplit=3, accumulate=1, bias=True),
          C("kq_asum_split3_deferred", "kq", 40, 100, 300, "TN", asum=True, nsplit=3, accumulate=2)]
    # gemm64<BK=64>: more than GEMM_KQ_MAX workgroups (3 x 2 x 86 = 516)
    t += [C("g64_nn", "g64_bk64", 130, 70, 100, "NN", nbatch=86),
          C("g64_nt_bias_relu_acc", "g64_bk64", 130, 70, 100, "NT", nbatch=86, bias_b=True, relu=1, accumulate=1, gap=True),
          C("g64_nt_misaligned", "g64_bk64", 130, 70, 100, "NT", nbatch=86, misalign=True),
          C("g64_tn_scn2", "g64_bk64", 130, 70, 100, "TN", nbatch=86, scn=2),
          C("g64_tt_ccol", "g64_bk64", 130, 70, 100, "TT", nbatch=86, ccol=True, bias=True),
          C("g64_cmul", "g64_bk64", 130, 70, 100, "TN", nbatch=86, cmul=True, gap=True),
          C("g64_cmask", "g64_bk64", 130, 70, 100, "NT", nbatch=86, cmul=True, relu=2, accumulate=1),
          C("g64_pair", "g64_bk64", 5450, 70, 100, "NT", nbatch=3, pair=True, bias_b=True, relu=1),
          C("g64_split2", "g64_bk64+reduce", 130, 70, 200, "TN", nbatch=43, nsplit=2, bias=True, relu=1, accumulate=1)]
    # gemm128_nt: 128-aligned Linear form that the tile kernels do not take (K no multiple of 64)
    t += [C("g128nt_128x128x16", "g128nt", 128, 128, 16, "NT", bias=True, relu=1),
          C("g128nt_256x128x80", "g128nt", 256, 128, 80, "NT", bias=True, relu=1),
          C("g128nt_plain", "g128nt", 128, 256, 48, "NT")]
    # tile kernels, 64x64
    t += [C("tile64_nt_64", "tile64", 64, 64, 64, "NT"),
          C("tile64_nt_192x128x128", "tile64", 192, 128, 128, "NT", bias=True, relu=1, accumulate=1),
          C("tile64_nn_1024", "tile64", 1024, 1024, 64, "NN", bias=True),
          C("tile64_tn_1024", "tile64", 1024, 1024, 64, "TN", accumulate=1),
          C("tile64_tt_1024", "tile64", 1024, 1024, 64, "TT", relu=1),
          C("tile64_split4_reduce", "tile64+reduce", 512, 512, 256, "TN", nsplit=4, bias=True, relu=1, accumulate=1),
          C("tile64_split4_deferred", "tile64", 512, 512, 256, "NN", nsplit=4, accumulate=2),
          C("tile64_nbatch2_bias_b", "tile64", 128, 64, 64, "NT", nbatch=2, bias_b=True, gap=True, relu=1)]
    # slabs of several batch entries through the reducer; the 128x128 grids in front of the reducer
    t += [C("tile64_split2_nbatch2_reduce", "tile64+reduce", 512, 512, 128, "TN", nsplit=2, nbatch=2, gap=True, bias=True, relu=1),
          C("tile128_split2_reduce", "tile128+reduce", 1024, 1536, 128, "TN", nsplit=2, accumulate=1),
          C("persist_whole_split4_reduce", "persist_whole+reduce", 2048, 2048, 512, "NT", nsplit=4, bias=True, relu=1, accumulate=1)]
    t += [C("tile64_pair", "tile64", 128, 64, 64, "NT", nbatch=2, pair=True, bias_b=True, relu=1)]
    # tile kernels, 128x128 on the plain grid (192 units, K <= 128)
    t += [C("tile128_nt", "tile128", 2048, 1536, 64, "NT", bias=True, relu=1),
          C("tile128_nn_acc", "tile128", 2048, 1536, 64, "NN", accumulate=1)]
    # the persistent 128x128 walk: 540 units (28 cut into halves), 783 units (remainder 271: whole tiles), 1024 units (no remainder)
    t += [C("persist_halves_nt", "persist_halves", 3456, 2560, 192, "NT", bias=True, relu=1),
          C("persist_halves_tn_acc", "persist_halves", 3456, 2560, 192, "TN", accumulate=1),
          C("persist_whole_783_acc", "persist_whole", 3456, 3712, 192, "NT", accumulate=1),
          C("persist_whole_1024", "persist_whole", 4096, 4096, 192, "NN", bias=True, relu=1)]
    # 320x256 tiles by LDS-DMA: whole rounds of 256 tiles
    t += [C("big_5120x4096x64", "big", 5120, 4096, 64, "NT"),
          C("big_nbatch2_bias_b", "big", 2560, 4096, 128, "NT", nbatch=2, bias_b=True),
          C("big_pair", "big", 2560, 4096, 128, "NT", nbatch=2, pair=True, bias_b=True),
          C("big_slabs_2", "big_slabs", 5120, 2048, 128, "NT", nsplit=2, accumulate=2),
          C("big_slabs_4", "big_slabs", 2560, 2048, 256, "NT", nsplit=4, accumulate=2)]
    return t


def _refusals():
    C = Case
    small = dict(M=70, N=33, K=100)
    r = [C("refuse_null_A", "refused", orient="NN", override={"A": None}, **small),
         C("refuse_M0", "refused", orient="NN", override={"M": 0}, **small),
         C("refuse_nsplit0", "refused", orient="NN", override={"nsplit": 0}, **small),
         C("refuse_deferred_nsplit1", "refused", orient="NN", accumulate=2, **small),
         C("refuse_deferred_nbatch2", "refused", 70, 33, 300, "NN", accumulate=2, nsplit=2, nbatch=2),
         C("refuse_deferred_bias", "refused", 70, 33, 300, "NN", accumulate=2, nsplit=2, bias=True),
         C("refuse_deferred_relu", "refused", 70, 33, 300, "NN", accumulate=2, nsplit=2, relu=1),
         C("refuse_cmul_nsplit2", "refused", 70, 33, 300, "NN", cmul=True, nsplit=2),
         C("refuse_relu2_without_cmul", "refused", orient="NN", override={"relu": 2}, **small),
         C("refuse_relu3", "refused", orient="NN", override={"relu": 3}, **small),
         C("refuse_relu3_cmul", "refused", orient="NN", cmul=True, override={"relu": 3}, **small),
         C("refuse_bias_b_nsplit2", "refused", 70, 33, 300, "NN", bias_b=True, nsplit=2, nbatch=2),
         C("refuse_null_ws", "refused", 70, 33, 300, "NN", nsplit=2, override={"splitk_ws": None}),
         C("refuse_null_ws_tile_shape", "refused", 512, 512, 256, "TN", nsplit=4, override={"splitk_ws": None}),
         C("refuse_asum_chunk48", "refused", 70, 33, 100, "TN", nsplit=3, asum=True),
         C("refuse_asum_516_workgroups", "refused", 130, 70, 100, "TN", nbatch=86, asum=True)]
    return r


def _groups():
    """(name, expected group_path_of, entries).  Entries of one group share an orientation unless the name says otherwise."""
    C = Case
    g = [("group_n2", "group", [C("gr2_a", "kq", 70, 33, 100, "TN", bias=True), C("gr2_b", "kq", 40, 100, 64, "TN", asum=True)])]
    shapes = [(33, 31, 64), (70, 33, 100), (1, 40, 65), (130, 70, 127), (40, 1, 128), (37, 35, 129), (40, 100, 100), (96, 160, 64),
              (65, 65, 200), (32, 32, 96)]
    opts = [dict(), dict(bias=True, relu=1, accumulate=1), dict(nbatch=3, gap=True, bias_b=True), dict(cmul=True), dict(asum=True),
            dict(accumulate=1), dict(asum=True, accumulate=1), dict(nbatch=2, cmul=True, gap=True), dict(scn=2, relu=1), dict(ccol=True)]
    for o in ("TN", "NN", "TT"):
        g.append(("group_n10_" + o.lower(), "group", [C("gr10%s_%d" % (o, i), "kq", M, N, K, o, **kw)
                                                      for i, ((M, N, K), kw) in enumerate(zip(shapes, opts))]))
    g.append(("group_n11_falls_back", "fallback", [C("gr11_%d" % i, "kq", 33 + i, 31, 64 + i, "TN", bias=bool(i & 1)) for i in range(11)]))
    g.append(("group_mixed_orientation_falls_back", "fallback",
              [C("grmix_a", "kq", 70, 33, 100, "TN"), C("grmix_b", "kq", 70, 33, 100, "NN", asum=True)]))
    g.append(("group_nt_entry_falls_back", "fallback",
              [C("grnt_a", "kq", 70, 33, 100, "NT", bias=True), C("grnt_b", "kq", 37, 35, 65, "NT")]))
    g.append(("group_relu2_entry_falls_back", "fallback",
              [C("grmask_a", "kq", 70, 33, 100, "TN", cmul=True, relu=2), C("grmask_b", "kq", 40, 100, 64, "TN", accumulate=1)]))
    g.append(("group_split_entry_falls_back", "fallback",
              [C("grsplit_a", "kq+reduce", 70, 33, 300, "TN", nsplit=4, bias=True), C("grsplit_b", "g64_bk16", 70, 33, 17, "TN")]))
    return g


def _group_refusals():
    """Groups with an entry mmego_gemm refuses: bad argument whether or not the rest could share a launch, and nothing is written."""
    C = Case
    ok = lambda n: C(n, "kq", 70, 33, 100, "TN", bias=True)
    return [("group_refuse_null_A", [ok("grr0_a"), C("grr0_b", "refused", 40, 100, 64, "TN", override={"A": None})]),
            ("group_refuse_relu3", [ok("grr1_a"), C("grr1_b", "refused", 40, 100, 64, "TN", override={"relu": 3})]),
            ("group_refuse_relu2_without_cmul", [ok("grr2_a"), C("grr2_b", "refused", 40, 100, 64, "TN", override={"relu": 2})]),
            ("group_refuse_deferred_unsplit", [ok("grr3_a"), C("grr3_b", "refused", 40, 100, 64, "TN", accumulate=2)]),
            ("group_refuse_last_of_fallback", [C("grr4_a", "kq", 70, 33, 100, "NT"), C("grr4_b", "refused", 40, 100, 64, "NT",
                                                                                       override={"nsplit": 0})])]


CASES = _cases()
REFUSALS = _refusals()
GROUPS = _groups()
GROUP_REFUSALS = _group_refusals()

# the options of the issue's list and the paths whose launcher accepts them: the tile kernels and gemm128_nt take none of them
# (cmul, asum or a strided C send a product to the strided kernels), asum is the K-quartered kernel's alone
OPTION_PATHS = {"cmul": ("kq", "g64_bk16", "g64_bk64"), "cmask": ("kq", "g64_bk16", "g64_bk64"),
                "cmul_nbatch": ("kq", "g64_bk16", "g64_bk64"), "strided_c": ("kq", "g64_bk16", "g64_bk64"),
                "asum": ("kq",), "asum_accumulate": ("kq",), "asum_nsplit": ("kq",), "asum_deferred": ("kq",),
                "relu_accumulate_bias": ("kq", "g64_bk16", "g64_bk64", "tile64")}


def kernel_of(label):
    return label.replace("+reduce", "")


def bf16_typical_error(K):
    """Typical error per output of a product of unit-normal operands when ONE operand is rounded to bf16 (relative rounding error
    uniform in +-2^-9, rms 2^-9 / sqrt(3) ~ 2^-9 0.6 per term, K independent terms)."""
    return 2.0 ** -9 * 0.6 * math.sqrt(K)
