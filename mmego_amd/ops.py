"""Typed host wrappers over the C ABI: shape/stride/dtype checks on the host, then one kernel launch.

Every function here runs on the GPU through libmmego_hip.so; nothing computes with torch ops.  Tensors
are fp32 CUDA(HIP) tensors; 2-D arguments may be strided views (e.g. a column slice of a wider buffer,
or ``W.t()``) -- the element strides go straight to the kernel.
"""
import os as _os

import numpy as np
import torch

from . import hip


def _chk(t, nd=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise TypeError("expected an fp32 device tensor, got %r" % (type(t),))
    if nd is not None and t.dim() != nd:
        raise ValueError("expected %d-D tensor, got shape %s" % (nd, tuple(t.shape)))
    return t


def _rows(t):
    """2-D row view [rows, C] with unit column stride of a contiguous-by-rows tensor."""
    _chk(t, 2)
    if t.stride(1) != 1:
        raise ValueError("row tensor needs unit column stride")
    return t


class Arena:
    """Named scratch buffers that persist across calls (static addresses: HIP-graph friendly).

    A buffer is never replaced: asking for a known name with another shape (a net used at a second minibatch size -- the short
    last minibatch of an epoch, an evaluation pass) creates a second buffer beside the first.  Captured HIP graphs keep replaying
    on the addresses they were captured with, so freeing or recycling a buffer they use would let them scribble over whatever
    the allocator puts there next."""

    def __init__(self, device):
        self.device = device
        self.bufs = {}

    def get(self, key, shape, dtype=torch.float32, zero=False):
        shape = tuple(int(s) for s in shape)
        slot = (key, shape, dtype)
        t = self.bufs.get(slot)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self.bufs[slot] = t
        if zero:
            fill(t, 0.0) if dtype == torch.float32 else t.zero_()
        return t

    def has(self, key):
        return any(k[0] == key for k in self.bufs)


_scratch = {}
_retired = []

_capture_origin = {"stream": None}


class capture:
    """`with ops.capture(graph[, stream=...])`: torch.cuda.graph plus the bookkeeping of the capture's ORIGIN stream.

    On this ROCm an event recorded on a stream that was itself forked from the capturing stream, and waited on by another
    non-origin stream, aborts the process at capture (scripts/repro_nested_capture_fork.py), so code that wants a side stream
    under capture may only fork from the origin (capture_can_fork()).  The origin is known exactly between the begin and the
    end of THIS context -- set on entry, cleared on exit, never left behind for a later capture -- and the engines only read
    it.  A capture started any other way (plain torch.cuda.graph) has no recorded origin: capture_can_fork() is False there
    and every caller takes its single-chain form."""

    def __init__(self, graph, **kw):
        self._ctx = torch.cuda.graph(graph, **kw)

    def __enter__(self):
        if _capture_origin["stream"] is not None:
            raise RuntimeError("ops.capture does not nest")
        self._ctx.__enter__()
        _capture_origin["stream"] = torch.cuda.current_stream().cuda_stream
        return self

    def __exit__(self, et, ev, tb):
        _capture_origin["stream"] = None
        return self._ctx.__exit__(et, ev, tb)


_no_fork = [0]


class no_fork:
    """`with ops.no_fork()`: every fork site of the package (blocks.lstm_recurrence's two chains, the engines' stage branches) takes
    its single-chain form -- whatever is launched inside runs as ONE dependency chain on the current stream.  The engines of
    train_step.py open it whenever a net of theirs runs bf16-MFMA kernels (precision "split3" / "bf16"): no other kernel is
    then ever resident on a CU beside a bf16-MFMA workgroup."""

    def __enter__(self):
        _no_fork[0] += 1
        return self

    def __exit__(self, et, ev, tb):
        _no_fork[0] -= 1
        return False


def capture_can_fork():
    """True when a side stream may be forked from the current stream: always when running eagerly; under graph capture only on
    the origin stream of an ops.capture context; never inside ops.no_fork()."""
    if _no_fork[0]:
        return False
    if not torch.cuda.is_current_stream_capturing():
        return True
    return _capture_origin["stream"] is not None and torch.cuda.current_stream().cuda_stream == _capture_origin["stream"]


def scratch(device, n):
    """Grow-only fp32 scratch per (device, stream) (split-K slabs, reduction partials).  Stream-ordered reuse is safe."""
    key = (str(device), torch.cuda.current_stream().cuda_stream)
    t = _scratch.get(key)
    if t is None or t.numel() < n:
        if t is not None:
            _retired.append(t)          # captured graphs may still replay on the smaller buffer: never hand its memory back
        t = torch.empty(max(int(n), 1 << 20), dtype=torch.float32, device=device)
        _scratch[key] = t
    return t


def mm(A, B, C, bias=None, relu=False, accumulate=False, nsplit=1, cmul=None, asum=None, cmask=None):
    """C[M,N] (+)= A[M,K] @ B[K,N] (+bias)(relu), then (*= cmul) or (= 0 where cmask <= 0) -- cmul / cmask: a tensor with C's
    shape and strides; A, B, C are 2-D views with arbitrary strides.  asum [M] (+)= row sums of A (see asum_ok)."""
    if cmask is not None:
        if cmul is not None or relu:
            raise ValueError("mm: cmask excludes cmul and relu")
        cmul, relu = cmask, 2
    _chk(A, 2), _chk(B, 2), _chk(C, 2)
    M, K = A.shape
    K2, N = B.shape
    if K2 != K or tuple(C.shape) != (M, N):
        raise ValueError("mm shape mismatch %s @ %s -> %s" % (tuple(A.shape), tuple(B.shape), tuple(C.shape)))
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        raise ValueError("bias must be contiguous with N elements")
    ws = None
    if nsplit > 1:
        ws = scratch(A.device, nsplit * (M * N + (M if asum is not None else 0)))
    if asum is not None and (asum.numel() != M or not asum.is_contiguous() or not asum_ok(M, N, K, nsplit, over_tile=True)):
        raise ValueError("mm: asum needs M contiguous elements and a small-product shape (ops.asum_ok)")
    if cmul is not None and (tuple(cmul.shape) != (M, N) or cmul.stride() != C.stride() or nsplit > 1):
        raise ValueError("mm: cmul needs C's shape and strides, and an unsplit product")
    hip.call("gemm", A, A.stride(0), A.stride(1), B, B.stride(0), B.stride(1), C, C.stride(0), C.stride(1), bias,
             M, N, K, 1, 0, 0, 0, int(relu), int(accumulate), ws, nsplit, 0, cmul, asum)
    return C


def bmm(A, B, C, accumulate=False, bias=None):
    """Batched C[b] (+)= A[b] @ B[b] (+ bias[n]); 3-D views, batch stride may be 0 (broadcast operand)."""
    _chk(A, 3), _chk(B, 3), _chk(C, 3)
    nb, M, K = A.shape
    if B.shape[0] != nb or C.shape[0] != nb or B.shape[1] != K or tuple(C.shape[1:]) != (M, B.shape[2]):
        raise ValueError("bmm shape mismatch")
    if bias is not None and (bias.numel() != B.shape[2] or not bias.is_contiguous()):
        raise ValueError("bias must be contiguous with N elements")
    hip.call("gemm", A, A.stride(1), A.stride(2), B, B.stride(1), B.stride(2), C, C.stride(1), C.stride(2), bias,
             M, B.shape[2], K, nb, A.stride(0), B.stride(0), C.stride(0), 0, int(accumulate), None, 1, 0, None, None)
    return C


def mm_two(A0, B0, C0, A1, B1, C1, bias0=None, bias1=None, cmul0=None, cmul1=None):
    """C0 = A0 @ B0 (+ bias0)(* cmul0) and C1 = A1 @ B1 (+ bias1)(* cmul1) -- two INDEPENDENT products of one shape -- as ONE batched
    launch: the batch strides are the distances between the operands (any two fp32 tensors are a whole number of elements apart).  The
    multipliers must lie as far apart as the outputs (two halves of one buffer).  Falls back to two launches when the layouts differ."""
    same = (A0.shape == A1.shape and B0.shape == B1.shape and C0.shape == C1.shape and A0.stride() == A1.stride() and B0.stride() == B1.stride()
            and C0.stride() == C1.stride() and (bias0 is None) == (bias1 is None) and (cmul0 is None) == (cmul1 is None))
    dA, dB, dC = A1.data_ptr() - A0.data_ptr(), B1.data_ptr() - B0.data_ptr(), C1.data_ptr() - C0.data_ptr()
    if same and cmul0 is not None:
        same = (cmul0.shape == C0.shape and cmul1.shape == C0.shape and cmul0.stride() == C0.stride() and cmul1.stride() == C0.stride()
                and cmul1.data_ptr() - cmul0.data_ptr() == dC)
    if same and bias0 is not None:
        same = bias0.is_contiguous() and bias1.is_contiguous() and bias0.numel() == B0.shape[1] == bias1.numel()
    if not same or dA % 16 or dB % 16 or dC % 16:
        mm(A0, B0, C0, bias=bias0, cmul=cmul0)
        mm(A1, B1, C1, bias=bias1, cmul=cmul1)
        return False
    _chk(A0, 2), _chk(B0, 2), _chk(C0, 2), _chk(A1, 2), _chk(B1, 2), _chk(C1, 2)
    M, K = A0.shape
    K2, N = B0.shape
    if K2 != K or tuple(C0.shape) != (M, N):
        raise ValueError("mm_two shape mismatch")
    dbias = (bias1.data_ptr() - bias0.data_ptr()) // 4 if bias0 is not None else 0
    hip.call("gemm", A0, A0.stride(0), A0.stride(1), B0, B0.stride(0), B0.stride(1), C0, C0.stride(0), C0.stride(1), bias0,
             M, N, K, 2, dA // 4, dB // 4, dC // 4, 0, 0, None, 1, dbias, cmul0, None)
    return True


def linear_pair(x, W0, W1, b0, b1, out, ncol):
    """out[:, :ncol] = x W0^T + b0 and out[:, ncol:2 ncol] = x W1^T + b1 as ONE batched product (the two directions' input
    projections of a BiLSTM layer: 2 x 1280 tiles = exactly five rounds of the persistent GEMM grid instead of 2 x 2.5)."""
    _chk(x, 2), _chk(out, 2)
    rows, K = x.shape
    ok = (W0.shape == W1.shape == (ncol, K) and W0.is_contiguous() and W1.is_contiguous() and b0.is_contiguous() and b1.is_contiguous()
          and x.stride(1) == 1 and out.stride(1) == 1 and out.shape[1] >= 2 * ncol)
    dW, dB = (W1.data_ptr() - W0.data_ptr()) // 4, (b1.data_ptr() - b0.data_ptr()) // 4
    if not ok or (W1.data_ptr() - W0.data_ptr()) % 16 or (b1.data_ptr() - b0.data_ptr()) % 4:
        linear(x, W0, b0, out[:, :ncol])
        linear(x, W1, b1, out[:, ncol:2 * ncol])
        return out
    hip.call("gemm", x, x.stride(0), 1, W0, 1, K, out, out.stride(0), 1, b0, rows, ncol, K, 2, 0, dW, ncol, 0, 0, None, 1, dB, None, None)
    return out


def stacked(a, b):
    """One [na + nb, ...] view over ``a`` and ``b`` when ``b`` sits directly behind ``a`` in memory (two tensors laid out back to
    back in a flat parameter / gradient buffer: params.FlatParams, a module's flat_param_order), else None."""
    if (a.dtype != b.dtype or tuple(a.shape[1:]) != tuple(b.shape[1:]) or not a.is_contiguous() or not b.is_contiguous()
            or b.data_ptr() != a.data_ptr() + a.numel() * a.element_size()
            or a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()):     # (neighbours by chance in the allocator are not one buffer)
        return None
    return torch.as_strided(a.detach(), (a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), a.stride())


def linear(x, W, b, out, relu=False):
    """out[rows,N] = x[rows,K] @ W[N,K]^T + b"""
    return mm(x, W.view(W.shape[0], -1).t(), out, bias=b, relu=relu)


_SPLIT_K_MIN = 128          # k per slab at least
_SPLIT_K_FROM = 1024        # split from this K on


def pick_split(M, N, K):
    """Split-K factor of a weight-gradient product: these have few output tiles and a long K (the batch rows), and a
    workgroup's k-loop is latency-bound per 64-k step, so K is cut down to one or two steps per workgroup as long as the
    grid stays within ~2 workgroups per CU."""
    if K <= _SPLIT_K_FROM:
        return 1        # short K: the K-quartered small-product kernel does it in one launch (no slab-reduce launch behind it)
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    want = max(1, 512 // tiles)
    return int(max(1, min(want, K // _SPLIT_K_MIN)))


def chain_split(M, N, K):
    """Split-K factor for a product on a serial critical path (the recurrent dh = dgates . W_hh of the LSTM backward): few
    output tiles and a long K, so the K range is cut until about two workgroups per CU are busy (>= 512 k per slab)."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    return int(max(1, min(512 // max(tiles, 1), K // 512)))


_KQ_MAX = 512               # gemm.hip GEMM_KQ_MAX
_TILE_MIN_OTHER = 256       # gemm.hip GEMM_TILE_MIN_OTHER
_PAIR_SPLIT_WGS = 512


def asum_ok(M, N, K, nsplit, nbatch=1, over_tile=False):
    """Whether mmego_gemm takes the K-quartered small-product kernel for this shape (its dispatch rule, gemm.hip), the one that
    can return the row sums of its A operand beside the product."""
    kchunk = -(-(-(-K // nsplit)) // 16) * 16
    wgs64 = ((M + 63) // 64) * ((N + 63) // 64) * nsplit * nbatch
    tile = M % 64 == 0 and N % 64 == 0 and K % 64 == 0 and (M // 64) * (N // 64) * nsplit * nbatch >= _TILE_MIN_OTHER
    return wgs64 <= _KQ_MAX and kchunk >= 64 and (over_tile or not tile) and M * N < (1 << 16)


def grad_weight(dY, X, dW, db=None, prefer_fused=False):
    """dW[N,K] = dY[rows,N]^T @ X[rows,K]  (fixed-order split over rows); db[N] (optional) = column sums of dY, the bias
    gradient: from the same launch where the product runs on the small-product kernel, a column-sum launch otherwise."""
    W2 = dW.view(dW.shape[0], -1)
    nsplit = pick_split(W2.shape[0], W2.shape[1], X.shape[0])
    # (prefer_fused: take the small-product kernel with the bias sums even where the tile kernel would be picked for the product
    # alone -- product + slab reduce instead of product + slab reduce + two column-sum launches)
    fused = db is not None and db.is_contiguous() and asum_ok(W2.shape[0], W2.shape[1], X.shape[0], nsplit, over_tile=prefer_fused)
    mm(dY.t(), X, W2, nsplit=nsplit, asum=db if fused else None)
    if db is not None and not fused:
        colsum(dY, db)
    return dW


class SlabList:
    """The deferred partial-product sums of one backward pass: split-K weight gradients (grad_weight_deferred), the temporal
    convolution's weight-gradient slabs and the edge-importance partials are left in buffers of their own (an Arena, not the shared
    scratch, which the next product would overwrite) and added by ONE mmego_slab_reduce launch at the end of the pass -- every such
    product used to be followed by a reduce launch of its own in the backward pass's dependent chain."""

    def __init__(self):
        self.items = []

    def add(self, ws, out, kind, nsplit, M, N, scm=0, taps=1, scale=None, asum=None):
        self.items.append(hip.Slab(hip.ptr(ws), hip.ptr(out), hip.ptr(scale), hip.ptr(asum), int(kind), int(nsplit), int(M), int(N), int(taps),
                                   int(scm)))

    def run(self):
        for i in range(0, len(self.items), 24):
            part = self.items[i:i + 24]
            arr = (hip.Slab * len(part))(*part)
            hip.call("slab_reduce", len(part), arr)
        self.items = []


def grad_weight_deferred(dY, X, dW, slabs, arena, key, db=None):
    """grad_weight whose split-K sum is left to ``slabs`` (a SlabList the caller runs at the end of its backward pass); db: the
    bias gradient rides along as the product's slab row sums where the small-product kernel takes the shape."""
    W2 = dW.view(dW.shape[0], -1)
    M, N = W2.shape
    K = X.shape[0]
    nsplit = pick_split(M, N, K)
    fused = db is not None and db.is_contiguous() and asum_ok(M, N, K, nsplit, over_tile=True)
    if nsplit == 1:
        mm(dY.t(), X, W2, asum=db if fused else None)
    else:
        _chk(dY, 2), _chk(X, 2)
        if dY.shape[0] != K or dY.shape[1] != M or X.shape[1] != N or not W2.is_contiguous():
            raise ValueError("grad_weight_deferred shape mismatch")
        ws = arena.get(key, (nsplit * (M * N + (M if fused else 0)),))
        hip.call("gemm", dY, dY.stride(1), dY.stride(0), X, X.stride(0), X.stride(1), W2, N, 1, None, M, N, K, 1, 0, 0, 0, 0, 2, ws, nsplit, 0,
                 None, db if fused else None)
        slabs.add(ws, W2, 0, nsplit, M, N, scm=N, asum=db if fused else None)
    if db is not None and not fused:
        colsum(dY, db)
    return dW


def grad_weight_pair(dY, ncol, X, dW0, dW1, X1=None, db=None):
    """dW0 = dY[:, :ncol]^T @ X and dW1 = dY[:, ncol:2 ncol]^T @ (X1 or X) as ONE batched product (the two directions' weight
    gradients of a BiLSTM layer; their slots in the flat gradient buffer are a fixed distance apart).  Falls back to two
    products when the layout does not allow it.  db [2 ncol] (optional, contiguous): the column sums of dY (both directions'
    bias gradients) from the same launch; -> True when db was written."""
    rows, K = X.shape
    Xb = X if X1 is None else X1
    W0, W1 = dW0.view(dW0.shape[0], -1), dW1.view(dW1.shape[0], -1)
    dist, xdist = W1.data_ptr() - W0.data_ptr(), Xb.data_ptr() - X.data_ptr()
    ok = (W0.shape == W1.shape == (ncol, K) and W0.is_contiguous() and W1.is_contiguous() and dY.stride(1) == 1 and X.stride(1) == 1
          and Xb.shape == X.shape and Xb.stride() == X.stride() and dist % 16 == 0 and xdist % 16 == 0)
    if ok and pick_split(ncol, K, rows) > 1:
        # long K (stage-1 IMU_Net: 10 240 rows): the two directions as one batched product keep twice the tiles in flight, so the
        # K range is cut half as often as for one direction alone (or not at all) -- one launch + at most one slab reduce instead
        # of two of each
        tiles = ((ncol + 63) // 64) * ((K + 63) // 64) * 2
        nsplit = int(max(1, min(_PAIR_SPLIT_WGS // tiles, rows // _SPLIT_K_MIN)))
        ws = scratch(dY.device, nsplit * 2 * ncol * K) if nsplit > 1 else None
        hip.call("gemm", dY, 1, dY.stride(0), X, X.stride(0), 1, W0, K, 1, None, ncol, K, rows, 2, ncol, xdist // 4, dist // 4, 0, 0, ws,
                 nsplit, 0, None, None)
        return False
    if not ok:
        grad_weight(dY[:, :ncol], X, dW0)
        grad_weight(dY[:, ncol:2 * ncol], Xb, dW1)
        return False
    fused = db is not None and db.is_contiguous() and db.numel() == 2 * ncol and asum_ok(ncol, K, rows, 1, nbatch=2)
    hip.call("gemm", dY, 1, dY.stride(0), X, X.stride(0), 1, W0, K, 1, None, ncol, K, rows, 2, ncol, xdist // 4, dist // 4, 0, 0, None, 1, 0,
             None, db if fused else None)
    return fused


def grad_input(dY, W, dX, accumulate=False, cmul=None, cmask=None):
    """dX[rows,K] (+)= dY[rows,N] @ W[N,K], then (*= cmul) or (= 0 where cmask <= 0: ReLU backward, cmask = the forward output)"""
    return mm(dY, W.view(W.shape[0], -1), dX, accumulate=accumulate, cmul=cmul, cmask=cmask)


def grad_input_slabs(arena, key, dY, W, dX):
    """dX[rows, In] = dY[rows, K] @ W[K, In] for outputs that are FEWER than 256 tiles of 320 x 256 (stage-1 IMU_Net training: 10 240 x
    {512, 1024} over K = 4096): against W^T both operands are k-contiguous, and with K cut into 256 / tiles slabs the product runs on
    gemm_tile_big_kernel, one workgroup per CU (r06: 0.85 instead of 0.52-0.63 of the fp32 peak on the 128 x 128 walk); the slabs are
    added in order by a streaming sum.  -> False (nothing done) where the shape does not fit."""
    rows, K = dY.shape
    W2 = W.view(W.shape[0], -1)
    In = W2.shape[1]
    if (rows % 320 or In % 256 or K % 64 or W2.shape[0] != K or dY.stride(1) != 1 or not W2.is_contiguous() or not dX.is_contiguous()
            or tuple(dX.shape) != (rows, In)):
        return False
    tiles = (rows // 320) * (In // 256)
    ns = 256 // tiles if tiles < 256 else 0
    if ns < 2 or tiles * ns != 256 or K // ns < 512:
        return False
    kchunk = -(-(-(-K // ns)) // 64) * 64
    if (ns - 1) * kchunk >= K or K - (ns - 1) * kchunk < 64:
        return False
    WT = arena.get("%s.wT" % key, (In, K))
    hip.call("transpose_batched", W2, WT, 1, K, In)
    ws = arena.get("%s.ws" % key, (ns * rows * In,))
    hip.call("gemm", dY, dY.stride(0), 1, WT, 1, K, dX, In, 1, None, rows, In, K, 1, 0, 0, 0, 0, 2, ws, ns, 0, None, None)
    hip.call("split3_slab_sum", ws, ns, rows * In, dX)
    return True


def colsum(X, out, accumulate=False, out2=None, scale=None):
    """out[c] (+)= sum_r X[r, c] (* scale[c], for up to 1024 rows); out2 (optional) gets a copy of the result."""
    X = _rows(X)
    rows, C = X.shape
    ws = scratch(X.device, C * hip.colstats_nblk(rows))
    hip.call("colsum", X, X.stride(0), rows, C, ws, out, out2, int(accumulate), scale)
    return out


def _pose_inputs(upper, lower, target):
    """The three joint tensors of the aligned metrics, [..., 15 | 8 | 21, 3] contiguous with the same leading shape; -> J."""
    lead = tuple(upper.shape[:-2])
    for t, n in ((upper, 15), (lower, 8), (target, 21)):
        if t is None:
            continue
        _chk(t)
        if tuple(t.shape) != lead + (n, 3) or not t.is_contiguous():
            raise ValueError("expected a contiguous %s tensor, got %s" % (lead + (n, 3), tuple(t.shape)))
    return 15 if lower is None else 21


def pose_errors_aligned_width(J, nthr):
    return hip.lib().mmego_pose_errors_aligned_width(int(J), int(nthr))


def pose_errors_aligned(upper, lower, target, thr, A):
    """Per-frame rows of mmego_pose_errors_aligned into A [F, >= 3 J + 3 + nthr] (root-relative, rigid-fit and similarity-fit joint
    errors; fit angle, shift and scale; PCK at the thresholds thr, a device tensor of metres, or None).  lower None: the 15 upper joints."""
    J = _pose_inputs(upper, lower, target)
    F = upper.numel() // 45
    nthr = 0 if thr is None else _chk(thr, 1).numel()
    A = _rows(A)
    if A.shape[0] != F or A.shape[1] < pose_errors_aligned_width(J, nthr) or (thr is not None and not thr.is_contiguous()):
        raise ValueError("pose_errors_aligned: A is %s for %d frames, %d joints and %d thresholds" % (tuple(A.shape), F, J, nthr))
    hip.call("pose_errors_aligned", upper, lower, target, F, thr, nthr, A, A.stride(0))
    return A


def pose_accel_errors(upper, lower, target, Acc):
    """Acc [B, >= J] <- the acceleration error per sequence and joint (mmego_pose_accel_errors); inputs [B, T, ., 3], T >= 3."""
    J = _pose_inputs(upper, lower, target)
    if upper.dim() != 4:
        raise ValueError("pose_accel_errors: inputs are [B, T, joints, 3]")
    B, T = upper.shape[0], upper.shape[1]
    Acc = _rows(Acc)
    if Acc.shape[0] != B or Acc.shape[1] < J:
        raise ValueError("pose_accel_errors: Acc is %s for %d sequences and %d joints" % (tuple(Acc.shape), B, J))
    hip.call("pose_accel_errors", upper, lower, target, B, T, Acc, Acc.stride(0))
    return Acc


BLEND_MAX_C = 64            # blend.hip BL_MAX_C: one lane per column
BONES_MAX_J = 21            # blend_bones.hip BB_MAX_J: one lane per joint
SMOOTH_MAX_H = 31           # smooth.hip SM_MAX_H: one lane per tap, 2 H + 1 <= 63
FLOOR_W = 22                # floor_math.h FLOOR_W: mmego_floor_stats' columns, 11 per foot


def _per_row(t, name, rows, dtype, device, who, kind=ValueError):
    """An optional per-row output: None, or one contiguous ``dtype`` word per row on the rows' device (``kind``: raised by anything else)."""
    if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype):
        raise kind("%s: %s is a %s device tensor" % (who, name, dtype))
    if t is not None and (t.dim() != 1 or t.numel() != rows or not t.is_contiguous() or t.device != device):
        raise ValueError("%s: %s is one contiguous %s word per row (%d), on the rows' device" % (who, name, dtype, rows))


def _seg_on(seg, rows, device, who):
    """seg of the filter and the floor launches: one int32 per row, a host array (uploaded) or a contiguous tensor on the rows' device."""
    if isinstance(seg, np.ndarray):
        if seg.dtype != np.int32 or seg.ndim != 1 or len(seg) != rows:
            raise ValueError("%s: seg is one int32 per row (%d), got %s %s" % (who, rows, seg.dtype, seg.shape))
        return torch.as_tensor(np.ascontiguousarray(seg)).to(device)
    if not (isinstance(seg, torch.Tensor) and seg.dtype == torch.int32 and seg.dim() == 1 and seg.numel() == rows and seg.is_contiguous()
            and seg.device == device):
        raise ValueError("%s: seg is one contiguous int32 per row (%d), a host array or a tensor on the rows' device" % (who, rows))
    return seg


def _rows_overlap(a, lda, b, ldb, rows, C):
    """True where the ``rows`` rows of C floats at tensor a (row stride lda) and at tensor b (row stride ldb) share a byte."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + 4 * ((rows - 1) * ldb + C) and b0 < a0 + 4 * ((rows - 1) * lda + C)


_tables_dev = {}         # (_upload_once's cache)


def _upload_once(device, *tables):
    """Host tables (numpy) on the device, uploaded once per content and device (cleared at 64 entries); an empty one as one zero row."""
    key = tuple((a.dtype.str, a.shape, a.tobytes()) for a in tables) + (str(device),)
    if key not in _tables_dev:
        if len(_tables_dev) >= 64:
            _tables_dev.clear()
        _tables_dev[key] = tuple(torch.as_tensor(a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)).to(device) for a in tables)
    return _tables_dev[key]


def _cover_on(cover, nrows, device):
    """The CSR cover (a data.DenseWindows / data.DensePlan, or its three host arrays cov_off, cov_row, cov_w) checked on the HOST against
    a source of ``nrows`` rows -- offsets ascending from 0 to the list's length, every row in [0, nrows) -- and uploaded (a plan object
    keeps its device copies).  -> (off, row, w, F)."""
    plan = cover if hasattr(cover, "cov_off") else None
    off, row, w = (plan.cov_off, plan.cov_row, plan.cov_w) if plan is not None else cover
    off, row, w = np.asarray(off), np.asarray(row), np.asarray(w)
    if off.dtype != np.int64 or row.dtype != np.int32 or w.dtype != np.float32 or off.ndim != 1 or row.ndim != 1 or w.ndim != 1:
        raise TypeError("blend_windows: the cover is int64 offsets, int32 rows and fp32 weights")
    if len(off) < 2 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != len(row) or len(row) != len(w):
        raise ValueError("blend_windows: the cover's offsets do not ascend from 0 to the length of its row list")
    if len(row) and (row.min() < 0 or row.max() >= nrows):
        raise IndexError("blend_windows: the cover names rows outside the %d source rows" % nrows)
    cache = plan.__dict__.setdefault("_cover_dev", {}) if plan is not None and hasattr(plan, "__dict__") else {}
    dev = cache.get(str(device))
    if dev is None:
        one = lambda a: torch.as_tensor(np.ascontiguousarray(a) if len(a) else np.zeros(1, a.dtype)).to(device)     # (an empty list: still an address)
        dev = cache[str(device)] = (one(off), one(row), one(w))
    return dev + (len(off) - 1,)


def blend_windows(src, cover, dst, spread=None):
    """dst[f, :C] = the weighted mean of the rows of src [nrows, C] that cover frame f (mmego_blend_windows: double inside, CSR order; a
    frame without cover gets zeros); spread [F] (optional, C % 3 == 0): the weighted RMS distance of those rows' joints from the blend.
    ``cover``: the plan object (cov_off, cov_row, cov_w as host arrays) or the three arrays; it is checked on the host first.  dst may be
    wider than C: its other columns stay."""
    _chk(src, 2)
    dst = _rows(dst)
    nrows, C = src.shape
    if not src.is_contiguous() or not 1 <= C <= BLEND_MAX_C:
        raise ValueError("blend_windows needs a contiguous source of 1 to %d columns, got %s" % (BLEND_MAX_C, tuple(src.shape)))
    off, row, w, F = _cover_on(cover, nrows, src.device)
    if dst.shape[0] != F or dst.shape[1] < C or (F > 1 and dst.stride(0) < C):
        raise ValueError("blend_windows: dst is %s for %d frames of %d columns" % (tuple(dst.shape), F, C))
    _per_row(spread, "spread", F, torch.float32, src.device, "blend_windows", kind=TypeError)
    if spread is not None and C % 3:
        raise ValueError("blend_windows: spread is one contiguous float per frame, of rows of 3-vectors")
    hip.call("blend_windows", src, nrows, C, off, row, w, F, dst, max(dst.stride(0), C), spread)
    return dst


def colsum_phase(X, period, out):
    """out[p, c] = sum of X[r, c] over the rows r = p (mod period) (mmego_colsum_phase): X [rows, C <= 64], rows % period == 0,
    out [period, >= C]."""
    X, out = _rows(X), _rows(out)
    rows, C = X.shape
    period = int(period)
    if not 1 <= period <= 64 or rows < 1 or rows % period or not 1 <= C <= BLEND_MAX_C:
        raise ValueError("colsum_phase: %d rows of %d columns do not fold by a period of %d" % (rows, C, period))
    if out.shape[0] != period or out.shape[1] < C:
        raise ValueError("colsum_phase: out is %s for %d phases of %d columns" % (tuple(out.shape), period, C))
    hip.call("colsum_phase", X, max(X.stride(0), C), rows, C, period, out, max(out.stride(0), C))
    return out


GROUPS_MAX_G = 65535        # breakdown.hip BD_MAX_G: one workgroup per group
GROUPS_MAX_ROWS = 1 << 24   # breakdown.hip: a group's row count travels as a float
HIST_MAX_BINS = 4096        # breakdown.hip BD_MAX_BINS: one LDS counter per bin


def is_float32(v):
    """True where the finite float64 ``v`` is a float32 exactly."""
    with np.errstate(over="ignore"):
        return bool(np.isfinite(np.float32(v)) and float(np.float32(v)) == float(v))


def _group_table(X, group, G, who):
    """The table and the group ids of colsum_groups / hist_groups checked on the host: X [rows, C] fp32 with unit column stride, group one
    contiguous int32 per row on X's device (or None where ``who`` allows it).  -> (X, rows, C, G)."""
    X = _rows(X)
    rows, C = X.shape
    if isinstance(G, bool) or not isinstance(G, (int, np.integer)):
        raise TypeError("%s: G is an integer number of groups, got %r" % (who, G))
    if not 1 <= rows < GROUPS_MAX_ROWS or not 1 <= C <= BLEND_MAX_C or (rows > 1 and X.stride(0) < C):
        raise ValueError("%s: a table of 1 to %d rows of 1 to %d columns, got %s" % (who, GROUPS_MAX_ROWS - 1, BLEND_MAX_C, tuple(X.shape)))
    if not 1 <= G <= GROUPS_MAX_G:
        raise ValueError("%s: G lies in [1, %d], got %d" % (who, GROUPS_MAX_G, G))
    _per_row(group, "group", rows, torch.int32, X.device, who, kind=TypeError)
    return X, rows, C, int(G)


def colsum_groups(X, group, G, out, count=None):
    """out[g, c] = the sum of X[r, c] over the rows with group[r] == g (mmego_colsum_groups: double inside, a fixed order; a row whose id
    lies outside [0, G) is in no sum): X [rows, C <= 64], group [rows] int32 on the device, out [G, >= C] (its other columns stay), count
    [G] fp32 (optional) the groups' row counts."""
    if group is None:
        raise TypeError("colsum_groups: group is an int32 device tensor")
    X, rows, C, G = _group_table(X, group, G, "colsum_groups")
    out = _rows(out)
    if out.device != X.device or out.shape[0] != G or out.shape[1] < C or (G > 1 and out.stride(0) < C):
        raise ValueError("colsum_groups: out is %s for %d groups of %d columns" % (tuple(out.shape), G, C))
    _per_row(count, "count", G, torch.float32, X.device, "colsum_groups", kind=TypeError)
    hip.call("colsum_groups", X, max(X.stride(0), C), rows, C, group, G, out, max(out.stride(0), C), count)
    return out


def hist_groups(X, group, G, inv_width, nbins, hist, dropped, pool=True):
    """Integer histograms of the values of X [rows, C <= 64] by group (mmego_hist_groups; its comment is the binning recipe): a value x
    lands in bin (int)(x * inv_width) -- inv_width, the bins per unit of X, has to be a float32 exactly, it is what the kernel multiplies
    by -- the last of the ``nbins`` bins taking everything beyond, NaN and negative values counted in ``dropped``.  group None: all rows,
    G = 1.  pool: one histogram per group, hist [G, nbins] and dropped [G]; else one per group and column, hist [G, C, nbins] and
    dropped [G, C]; both contiguous int32 device tensors, every word of which is written."""
    X, rows, C, G = _group_table(X, group, G, "hist_groups")
    if group is None and G != 1:
        raise ValueError("hist_groups: without group ids there is one group, got G = %d" % G)
    if isinstance(nbins, bool) or not isinstance(nbins, (int, np.integer)):
        raise TypeError("hist_groups: nbins is an integer, got %r" % (nbins,))
    if not 1 <= nbins <= HIST_MAX_BINS:
        raise ValueError("hist_groups: nbins lies in [1, %d], got %d" % (HIST_MAX_BINS, nbins))
    if isinstance(inv_width, bool) or not isinstance(inv_width, (int, float, np.integer, np.floating)):
        raise TypeError("hist_groups: inv_width is a number, got %r" % (inv_width,))
    inv = float(inv_width)
    if not 0.0 < inv < float("inf") or not is_float32(inv):                   # (false for NaN as well)
        raise ValueError("hist_groups: inv_width is finite, > 0 and a float32 exactly, got %r" % (inv_width,))
    shape = (G, int(nbins)) if pool else (G, C, int(nbins))
    for t, name, want in ((hist, "hist", shape), (dropped, "dropped", shape[:-1])):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32):
            raise TypeError("hist_groups: %s is an int32 device tensor" % name)
        if tuple(t.shape) != want or not t.is_contiguous() or t.device != X.device:
            raise ValueError("hist_groups: %s is a contiguous %s on the table's device, got %s" % (name, want, tuple(t.shape)))
    hip.call("hist_groups", X, max(X.stride(0), C), rows, C, group, G, inv, int(nbins), int(bool(pool)), hist, dropped)
    return hist


def _bones_on(bones, bone_len, J, device, who):
    """The walk table ((child, parent) per bone, host integers) and the bone lengths checked on the HOST for rows of J joints -- every
    joint a child at most once, every parent a root or an earlier bone's child (so there is no cycle), the lengths finite and positive
    -- and uploaded once per table and device.  -> (bones int32 [NB, 2], bone_len fp32 [NB], NB)."""
    b = np.asarray(bones)
    L = np.asarray(bone_len.detach().cpu() if isinstance(bone_len, torch.Tensor) else bone_len)
    if b.size == 0:
        b = np.zeros((0, 2), dtype=np.int32)
    if b.ndim != 2 or b.shape[1] != 2 or not np.issubdtype(b.dtype, np.integer) or L.ndim != 1 or len(L) != len(b):
        raise ValueError("%s: bones is [NB, 2] integers of (child, parent) and bone_len one length per bone" % who)
    if not 1 <= J <= BONES_MAX_J or len(b) > J - 1:
        raise ValueError("%s: rows of %d joints with %d bones (1 to %d joints, at most one bone less)" % (who, J, len(b), BONES_MAX_J))
    if len(b) and (b.min() < 0 or b.max() >= J):
        raise IndexError("%s: the bones name joints outside the %d of a row" % (who, J))
    children = [int(c) for c in b[:, 0]]
    if len(set(children)) != len(children):
        raise ValueError("%s: a joint is the child of two bones" % who)
    placed = set(range(J)) - set(children)              # the roots
    for c, p in b.tolist():
        if p not in placed:
            raise ValueError("%s: bone (%d, %d) comes before its parent's own bone; the walk goes parents first" % (who, c, p))
        placed.add(c)
    L = L.astype(np.float32)
    if len(L) and not (np.isfinite(L).all() and (L > 0).all()):
        raise ValueError("%s: bone lengths have to be finite and positive" % who)
    return _upload_once(device, np.ascontiguousarray(b, dtype=np.int32), L) + (len(b),)


def blend_bones(src, cover, bones, bone_len, dst, spread=None, fallback=None):
    """dst[f, :3 J] = the bone-length-preserving blend of the rows of src [nrows, 3 J] (rigid skeletons of J <= 21 joints) that cover
    frame f (mmego_blend_bones; the recipe is in the header): roots as blend_windows blends them, every bone's direction blended over
    the cover, set to bone_len and laid along ``bones`` ([NB, 2] host integers (child, parent), parents first).  spread [F] (optional)
    as blend_windows', against the rigid positions; fallback [F] int32 (optional): the bones per frame whose blended direction was
    degenerate.  Cover, bones and lengths are checked on the host first; a refused call leaves every output untouched.  dst may be wider
    than 3 J: its other columns stay."""
    _chk(src, 2)
    dst = _rows(dst)
    nrows, C = src.shape
    if not src.is_contiguous() or C % 3 or not 1 <= C // 3 <= BONES_MAX_J:
        raise ValueError("blend_bones needs a contiguous source of 1 to %d 3-vectors a row, got %s" % (BONES_MAX_J, tuple(src.shape)))
    bd, ld, NB = _bones_on(bones, bone_len, C // 3, src.device, "blend_bones")
    off, row, w, F = _cover_on(cover, nrows, src.device)
    if dst.shape[0] != F or dst.shape[1] < C or (F > 1 and dst.stride(0) < C):
        raise ValueError("blend_bones: dst is %s for %d frames of %d columns" % (tuple(dst.shape), F, C))
    _per_row(spread, "spread", F, torch.float32, src.device, "blend_bones", kind=TypeError)
    _per_row(fallback, "fallback", F, torch.int32, src.device, "blend_bones")
    hip.call("blend_bones", src, nrows, C // 3, off, row, w, F, bd, ld, NB, dst, max(dst.stride(0), C), spread, fallback)
    return dst


def bone_length_dev(X, bones, bone_len, out):
    """out[r, b] = | |X[r, c_b] - X[r, p_b]| - bone_len[b] | (mmego_bone_length_dev): X [n, 3 J] rows of 3-vectors (a strided row view is
    fine), out [n, >= NB]; bones and lengths as blend_bones takes and checks them.  A per-row table for colsum."""
    X, out = _rows(X), _rows(out)
    n, C = X.shape
    if n < 1 or C % 3 or not 1 <= C // 3 <= BONES_MAX_J:
        raise ValueError("bone_length_dev needs rows of 1 to %d 3-vectors, got %s" % (BONES_MAX_J, tuple(X.shape)))
    bd, ld, NB = _bones_on(bones, bone_len, C // 3, X.device, "bone_length_dev")
    if NB < 1 or out.shape[0] != n or out.shape[1] < NB:
        raise ValueError("bone_length_dev: out is %s for %d rows of %d bones" % (tuple(out.shape), n, NB))
    hip.call("bone_length_dev", X, max(X.stride(0), C), n, C // 3, bd, ld, NB, out, max(out.stride(0), NB))
    return out


def blend_rot(src, q, Rh, cover, bones, rot_idx, body, dst, quat, spread=None, rot_spread=None, fallback=None):
    """dst[f, :3 J] = the blend in rotation space of the rows that cover frame f (mmego_blend_rot; the recipe is in the header): per bone
    the weighted chordal mean of the world rotations Rh^T q of the cover, the roots as blend_windows blends them, the rest bones ``body``
    laid along the means over ``bones``; quat [F, NB, 4] receives the means as unit quaternions (w, x, y, z) of canonical sign.
    src [nrows, 3 J] the rows' joints (J <= 21), q [nrows, NQ, 9] (or [nrows, NQ, 3, 3]) the rows' rotations, Rh [nrows, 9] (or
    [nrows, 3, 3]) the head rotation each row ran with; bones [NB, 2] host integers (child, parent), parents first, rot_idx [NB] host
    integers in [0, NQ), body [NB, 3] host floats with no zero vector.  spread [F] (optional) as blend_windows', against the rigid
    positions; rot_spread [F] (optional) the windows' weighted RMS rotational distance from the mean in radians; fallback [F] int32
    (optional) the bones per frame whose mean was degenerate.  Every tensor is contiguous float32 on src's device.  Cover, bones,
    rot_idx and body are checked on the host first; a refused call leaves every output untouched.  dst may be wider than 3 J: its other
    columns stay."""
    _chk(src, 2)
    dst = _rows(dst)
    nrows, C = src.shape
    if not src.is_contiguous() or C % 3 or not 2 <= C // 3 <= BONES_MAX_J:
        raise ValueError("blend_rot needs a contiguous source of 2 to %d 3-vectors a row, got %s" % (BONES_MAX_J, tuple(src.shape)))
    for name, t in (("q", q), ("Rh", Rh), ("quat", quat)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == src.device and t.is_contiguous()):
            raise ValueError("blend_rot: %s is a contiguous float32 tensor on the source's device" % name)
    if q.dim() not in (3, 4) or q.shape[0] != nrows or q.shape[1] < 1 or q.numel() != nrows * q.shape[1] * 9:
        raise ValueError("blend_rot: q is [%d, NQ, 9], one 3 x 3 rotation per row and bone, got %s" % (nrows, tuple(q.shape)))
    NQ = q.shape[1]
    if Rh.dim() not in (2, 3) or Rh.shape[0] != nrows or Rh.numel() != nrows * 9:
        raise ValueError("blend_rot: Rh is [%d, 9], one head rotation per row, got %s" % (nrows, tuple(Rh.shape)))
    bv = np.asarray(body.detach().cpu() if isinstance(body, torch.Tensor) else body)
    if bv.ndim != 2 or bv.shape[1] != 3 or bv.dtype.kind != "f":
        raise ValueError("blend_rot: body is [NB, 3] floats, one rest vector per bone")
    bv = np.ascontiguousarray(bv, dtype=np.float32)
    if not np.isfinite(bv).all():
        raise ValueError("blend_rot: bone lengths have to be finite and positive")
    bd, _, NB = _bones_on(bones, np.linalg.norm(bv.astype(np.float64), axis=1), C // 3, src.device, "blend_rot")
    if NB < 1:
        raise ValueError("blend_rot: at least one bone")
    ri = np.asarray(rot_idx)
    if ri.ndim != 1 or len(ri) != NB or not np.issubdtype(ri.dtype, np.integer):
        raise ValueError("blend_rot: rot_idx is one integer per bone (%d)" % NB)
    if ri.min() < 0 or ri.max() >= NQ:
        raise IndexError("blend_rot: rot_idx names rotations outside the %d of a row" % NQ)
    off, row, w, F = _cover_on(cover, nrows, src.device)
    if dst.shape[0] != F or dst.shape[1] < C or (F > 1 and dst.stride(0) < C):
        raise ValueError("blend_rot: dst is %s for %d frames of %d columns" % (tuple(dst.shape), F, C))
    if quat.numel() != F * NB * 4 or quat.shape[0] != F or quat.data_ptr() % 16:
        raise ValueError("blend_rot: quat is [%d, %d, 4], 16-byte aligned, got %s" % (F, NB, tuple(quat.shape)))
    _per_row(spread, "spread", F, torch.float32, src.device, "blend_rot", kind=TypeError)
    _per_row(rot_spread, "rot_spread", F, torch.float32, src.device, "blend_rot", kind=TypeError)
    _per_row(fallback, "fallback", F, torch.int32, src.device, "blend_rot")
    rd = _upload_once(src.device, np.ascontiguousarray(ri, dtype=np.int32), bv)
    hip.call("blend_rot", src, nrows, C // 3, q, NQ, Rh, off, row, w, F, bd, rd[0], rd[1], NB, dst, max(dst.stride(0), C), quat, spread,
             rot_spread, fallback)
    return dst


def _smooth_on(src, seg, weights, order, dst, moved, C_max, who):
    """What the two smoothing launches share, checked on the HOST: src [F, C] and dst [F, >= C] row tensors that share no byte, the
    weight table (host floats: odd length 2 H + 1 with H in [1, 31], every weight finite and > 0; uploaded once per table and device),
    order in {0, 1, 2}, seg (an int32 host array or device tensor of length F; a host array is uploaded), moved (optional): one
    contiguous float per frame, of rows of 3-vectors.  -> (seg, w, H, order, F, C, lds, ldd)."""
    src, dst = _rows(src), _rows(dst)
    F, C = src.shape
    if F < 1 or not 1 <= C <= C_max or (F > 1 and src.stride(0) < C):
        raise ValueError("%s needs a source of at least one row of 1 to %d columns, got %s" % (who, C_max, tuple(src.shape)))
    if dst.shape[0] != F or dst.shape[1] < C or (F > 1 and dst.stride(0) < C):
        raise ValueError("%s: dst is %s for %d frames of %d columns" % (who, tuple(dst.shape), F, C))
    lds, ldd = max(src.stride(0), C), max(dst.stride(0), C)
    if _rows_overlap(src, lds, dst, ldd, F, C):
        raise ValueError("%s: dst overlaps src; the filter reads the rows around the one it writes and cannot run in place" % who)
    wt = np.asarray(weights.detach().cpu() if isinstance(weights, torch.Tensor) else weights)
    if wt.ndim != 1 or wt.dtype.kind != "f" or len(wt) % 2 == 0 or not 1 <= len(wt) // 2 <= SMOOTH_MAX_H:
        raise ValueError("%s: the weights are a table of 2 H + 1 floats with H in [1, %d], got %s" % (who, SMOOTH_MAX_H, wt.shape))
    wt = np.ascontiguousarray(wt, dtype=np.float32)
    if not (np.isfinite(wt).all() and (wt > 0).all()):
        raise ValueError("%s: every weight has to be finite and > 0" % who)
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 0 <= order <= 2:
        raise ValueError("%s: order (the polynomial's degree) is 0, 1 or 2, got %r" % (who, order))
    seg = _seg_on(seg, F, src.device, who)
    _per_row(moved, "moved", F, torch.float32, src.device, who, kind=TypeError)
    if moved is not None and C % 3:
        raise ValueError("%s: moved is one contiguous float per frame, of rows of 3-vectors" % who)
    return seg, _upload_once(src.device, wt)[0], len(wt) // 2, int(order), F, C, lds, ldd


def smooth_frames(src, seg, weights, order, dst, moved=None):
    """dst[f, :C] = the zero-phase local-polynomial filter of the rows of src [F, C <= 64] along the frames (mmego_smooth_frames; the
    recipe is in the header): the weighted least-squares polynomial of degree min(order, valid taps - 1) through the rows f - H .. f + H
    of frame f's own segment, evaluated at f.  ``seg`` [F] int32 names every frame's segment (-1: none; such a frame, and one alone in
    its segment, keeps its row bit for bit); ``weights`` the 2 H + 1 tap weights (host floats, dense.smooth_weights); ``order`` 0, 1
    or 2.  moved [F] (optional, C % 3 == 0): the RMS distance over the joints between the filtered and the source row.  Everything is
    checked on the host first (ValueError); dst must not overlap src, and may be wider than C: its other columns stay."""
    seg, w, H, order, F, C, lds, ldd = _smooth_on(src, seg, weights, order, dst, moved, BLEND_MAX_C, "smooth_frames")
    hip.call("smooth_frames", src, lds, F, C, seg, w, H, order, dst, ldd, moved)
    return dst


def smooth_bones(src, seg, weights, order, walk, lengths, dst, moved=None, fallback=None):
    """The same filter for rows of rigid skeletons, src [F, 3 J] with J <= 21 (mmego_smooth_bones): the roots filtered as smooth_frames
    filters them, every bone's direction filtered, set to ``lengths`` and laid along ``walk`` ([NB, 2] host integers (child, parent),
    parents first; checked as blend_bones checks them) -- the filtered frames are rigid skeletons again.  fallback [F] int32 (optional):
    the bones per frame whose filtered direction cancelled and that kept the frame's own direction."""
    if src.dim() == 2 and src.shape[1] % 3:
        raise ValueError("smooth_bones needs rows of 3-vectors, got %s" % (tuple(src.shape),))
    seg, w, H, order, F, C, lds, ldd = _smooth_on(src, seg, weights, order, dst, moved, 3 * BONES_MAX_J, "smooth_bones")
    bd, ld, NB = _bones_on(walk, lengths, C // 3, src.device, "smooth_bones")
    _per_row(fallback, "fallback", F, torch.int32, src.device, "smooth_bones")
    hip.call("smooth_bones", src, lds, F, C // 3, seg, w, H, order, bd, ld, NB, dst, ldd, moved, fallback)
    return dst


def smooth_rot(src, quat, seg, weights, order, walk, body, dst, quat_out, moved=None, rot_moved=None, fallback=None):
    """The same filter in rotation space, for the rigid rows and quaternions blend_rot wrote (mmego_smooth_rot; the recipe is in the
    header): src [F, 3 J] with J <= 21, quat [F, NB, 4] the unit quaternions (w, x, y, z) of every bone's world rotation.  The roots are
    filtered as smooth_frames filters them; every bone's rotation becomes the proper rotation nearest sum_k c_k A_k over its valid taps
    -- at order 0 the weighted chordal mean of the neighbouring frames -- and the rest bones ``body`` ([NB, 3] host floats) are laid
    along ``walk`` ([NB, 2] host integers (child, parent), parents first; checked as blend_rot checks them).  dst [F, >= 3 J] receives
    the rigid filtered rows, quat_out [F, NB, 4] their quaternions in canonical sign; moved [F] (optional) as smooth_frames';
    rot_moved [F] (optional): the RMS angle over the bones, in radians, that the filter turned the frame; fallback [F] int32
    (optional): the bones per frame whose filtered rotation had no direction and that kept the frame's own.  Everything is checked on
    the host first; a refused call leaves every output untouched.  Neither output may overlap its input."""
    if src.dim() == 2 and src.shape[1] % 3:
        raise ValueError("smooth_rot needs rows of 3-vectors, got %s" % (tuple(src.shape),))
    seg, w, H, order, F, C, lds, ldd = _smooth_on(src, seg, weights, order, dst, moved, 3 * BONES_MAX_J, "smooth_rot")
    if C // 3 < 2:
        raise ValueError("smooth_rot needs rows of 2 to %d 3-vectors, got %s" % (BONES_MAX_J, tuple(src.shape)))
    for name, t in (("quat", quat), ("quat_out", quat_out)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == src.device and t.is_contiguous()):
            raise ValueError("smooth_rot: %s is a contiguous float32 tensor on the source's device" % name)
    bv = np.asarray(body.detach().cpu() if isinstance(body, torch.Tensor) else body)
    if bv.ndim != 2 or bv.shape[1] != 3 or bv.dtype.kind != "f":
        raise ValueError("smooth_rot: body is [NB, 3] floats, one rest vector per bone")
    bv = np.ascontiguousarray(bv, dtype=np.float32)
    if not np.isfinite(bv).all():
        raise ValueError("smooth_rot: bone lengths have to be finite and positive")
    bd, _, NB = _bones_on(walk, np.linalg.norm(bv.astype(np.float64), axis=1), C // 3, src.device, "smooth_rot")
    if NB < 1:
        raise ValueError("smooth_rot: at least one bone")
    for name, t in (("quat", quat), ("quat_out", quat_out)):
        if t.dim() != 3 or tuple(t.shape) != (F, NB, 4) or t.data_ptr() % 16:
            raise ValueError("smooth_rot: %s is [%d, %d, 4], 16-byte aligned, got %s" % (name, F, NB, tuple(t.shape)))
    if _rows_overlap(quat, 4 * NB, quat_out, 4 * NB, F, 4 * NB):
        raise ValueError("smooth_rot: quat_out overlaps quat; the filter reads the frames around the one it writes")
    _per_row(rot_moved, "rot_moved", F, torch.float32, src.device, "smooth_rot", kind=TypeError)
    _per_row(fallback, "fallback", F, torch.int32, src.device, "smooth_rot")
    hip.call("smooth_rot", src, lds, F, C // 3, quat, NB, seg, w, H, order, bd, _upload_once(src.device, bv)[0], dst, ldd, quat_out,
             moved, rot_moved, fallback)
    return dst


def one_euro_runs(seg):
    """The runs of the causal filter from the host int32 ``seg`` [F] (a frame's segment, -1: none): the maximal stretches of consecutive
    frames with the same segment, which partition [0, F).  -> (run_off [R + 1] int64 ascending from 0 to F, run_on [R] int32: 1 where the
    run's segment is >= 0 -- it is filtered --, 0 where it is an uncovered stretch -- its rows are copied)."""
    seg = np.asarray(seg)
    if seg.dtype != np.int32 or seg.ndim != 1 or len(seg) < 1:
        raise ValueError("one_euro_runs: seg is one int32 per frame, at least one, got %s %s" % (seg.dtype, seg.shape))
    first = np.concatenate([[0], np.flatnonzero(seg[1:] != seg[:-1]) + 1]).astype(np.int64)
    return np.concatenate([first, [len(seg)]]).astype(np.int64), (seg[first] >= 0).astype(np.int32)


def _one_euro_on(src, runs, fc, beta, dc, dst, moved, who):
    """What the two causal-filter launches share, checked on the HOST: src [F, 3 J] and dst [F, >= 3 J] row tensors that share no byte;
    runs = (run_off, run_on), host arrays as one_euro_runs returns them -- run_off int64 ascending from 0 to F with every run at least
    one frame, run_on int32 one per run; fc finite > 0, beta finite >= 0, dc finite > 0; moved (optional): one contiguous float per
    frame.  -> (run_off, run_on on the device, R, fc, beta, dc, F, C, lds, ldd)."""
    if not (isinstance(src, torch.Tensor) and isinstance(dst, torch.Tensor) and src.is_cuda and dst.is_cuda and src.dtype == torch.float32
            and dst.dtype == torch.float32 and src.device == dst.device):
        raise ValueError("%s: src and dst are fp32 tensors on one device" % who)
    if src.dim() != 2 or dst.dim() != 2 or src.stride(1) != 1 or dst.stride(1) != 1:
        raise ValueError("%s: src and dst are row tensors with unit column stride, got %s and %s" % (who, tuple(src.shape), tuple(dst.shape)))
    F, C = src.shape
    if F < 1 or C % 3 or not 1 <= C // 3 <= BONES_MAX_J or (F > 1 and src.stride(0) < C):
        raise ValueError("%s needs a source of at least one row of 1 to %d 3-vectors, got %s" % (who, BONES_MAX_J, tuple(src.shape)))
    if dst.shape[0] != F or dst.shape[1] < C or (F > 1 and dst.stride(0) < C):
        raise ValueError("%s: dst is %s for %d frames of %d columns" % (who, tuple(dst.shape), F, C))
    lds, ldd = max(src.stride(0), C), max(dst.stride(0), C)
    if _rows_overlap(src, lds, dst, ldd, F, C):
        raise ValueError("%s: dst overlaps src; the filter reads rows ahead of the one it writes and cannot run in place" % who)
    if not (isinstance(runs, (tuple, list)) and len(runs) == 2):
        raise ValueError("%s: runs is (run_off, run_on), as one_euro_runs returns them" % who)
    off, on = (np.asarray(a) for a in runs)
    if off.dtype != np.int64 or on.dtype != np.int32 or off.ndim != 1 or on.ndim != 1 or len(off) != len(on) + 1 or len(on) < 1:
        raise ValueError("%s: run_off is [R + 1] int64 and run_on [R] int32 with R >= 1, got %s %s and %s %s"
                         % (who, off.dtype, off.shape, on.dtype, on.shape))
    if off[0] != 0 or off[-1] != F or (np.diff(off) < 1).any():
        raise ValueError("%s: run_off does not ascend from 0 to the %d frames with every run at least one frame" % (who, F))
    par = []
    for name, v, low in (("fc (the minimum cutoff)", fc, "> 0"), ("beta", beta, ">= 0"), ("dc (the speed estimate's cutoff)", dc, "> 0")):
        ok = not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
        if not ok or v < 0 or (v == 0 and low == "> 0"):
            raise ValueError("%s: %s is a finite number %s, got %r" % (who, name, low, v))
        par.append(float(v))
    _per_row(moved, "moved", F, torch.float32, src.device, who)
    off_d, on_d = _upload_once(src.device, np.ascontiguousarray(off), np.ascontiguousarray(on))
    return (off_d, on_d, len(on)) + tuple(par) + (F, C, lds, ldd)


def one_euro(src, runs, fc, beta, dc, dst, moved=None):
    """dst[f, :3 J] = the one-euro filter of the rows of src [F, 3 J] (J <= 21 3-vectors a row) along the frames (mmego_one_euro; the
    recipe is in the header): a causal exponential low-pass per joint whose cutoff is fc + beta |dhat| cycles per frame, dhat the
    joint's own filtered speed (cutoff dc); frame f's row depends on no later frame.  ``runs`` = (run_off, run_on) from one_euro_runs:
    every filtered run starts from its own first frame, whose row is kept bit for bit, and a copy run keeps all its rows.  moved [F]
    (optional): the RMS distance over the joints between the filtered and the source row.  Everything is checked on the host first
    (ValueError); dst must not overlap src, and may be wider than 3 J: its other columns stay."""
    off, on, R, fc, beta, dc, F, C, lds, ldd = _one_euro_on(src, runs, fc, beta, dc, dst, moved, "one_euro")
    hip.call("one_euro", src, lds, F, C // 3, off, on, R, fc, beta, dc, dst, ldd, moved)
    return dst


def one_euro_bones(src, runs, fc, beta, dc, walk, lengths, dst, moved=None, fallback=None):
    """The same filter for rows of rigid skeletons (mmego_one_euro_bones): the roots filtered as one_euro filters them, every bone's
    vector child - parent filtered by the same recursion, set to ``lengths`` and laid along ``walk`` ([NB, 2] host integers (child,
    parent), parents first; checked as blend_bones checks them) -- the filtered frames are rigid skeletons again.  fallback [F] int32
    (optional): the bones per frame whose filtered vector vanished and that took the frame's own direction."""
    off, on, R, fc, beta, dc, F, C, lds, ldd = _one_euro_on(src, runs, fc, beta, dc, dst, moved, "one_euro_bones")
    bd, ld, NB = _bones_on(walk, lengths, C // 3, src.device, "one_euro_bones")
    _per_row(fallback, "fallback", F, torch.int32, src.device, "one_euro_bones")
    hip.call("one_euro_bones", src, lds, F, C // 3, off, on, R, fc, beta, dc, bd, ld, NB, dst, ldd, moved, fallback)
    return dst


def _floor_rows(t, name, rows, C, device, who, packed=False):
    """One row tensor of the floor launches, checked on the HOST: an fp32 device tensor [rows, >= C] on ``device`` with unit column
    stride and a row stride of at least its width (``packed``: exactly [rows, C], contiguous).  -> its row stride."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
        raise ValueError("%s: %s is a 2-D fp32 device tensor" % (who, name))
    if device is not None and t.device != device:
        raise ValueError("%s: %s lies on %s, the rows on %s" % (who, name, t.device, device))
    if rows is not None and t.shape[0] != rows:
        raise ValueError("%s: %s has %d rows for %d" % (who, name, t.shape[0], rows))
    if t.shape[0] < 1 or (t.shape[1] != C if packed else t.shape[1] < C):
        raise ValueError("%s: %s is %s, wanted at least one row of %s%d columns" % (who, name, tuple(t.shape), "" if packed else ">= ", C))
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) or (packed and not t.is_contiguous()):
        raise ValueError("%s: %s needs unit column stride and %s" % (who, name, "packed rows" if packed else "rows that do not overlap"))
    return max(t.stride(0), t.shape[1])


def _floor_metres(v, name, who, zero_ok):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0 or (v == 0 and not zero_ok):
        raise ValueError("%s: %s is a finite number of metres %s 0, got %r" % (who, name, ">=" if zero_ok else ">", v))
    return float(v)


def floor_stats(lo, tgt, ground, contact, seg, H, out):
    """out [rows, FLOOR_W] = the floor figures of both feet of every row (mmego_floor_stats; the columns are in the header): lo
    [rows, >= 24] the predicted lower joints, tgt [rows, >= 63] the 21-joint target, ground [rows, 4] the planes and contact [rows, 2]
    the recorded flags (fp32, packed), seg [rows] int32 (a host array or a device tensor; < 0: the row writes zeros), H > 0 the contact
    height in metres.  Everything is checked on the host first (ValueError).  The column sums are ops.colsum's."""
    who = "floor_stats"
    ldl = _floor_rows(lo, "lo", None, 24, None, who)
    rows, dev = lo.shape[0], lo.device
    ldt = _floor_rows(tgt, "tgt", rows, 63, dev, who)
    _floor_rows(ground, "ground", rows, 4, dev, who, packed=True)
    _floor_rows(contact, "contact", rows, 2, dev, who, packed=True)
    _floor_rows(out, "out", rows, FLOOR_W, dev, who, packed=True)
    seg = _seg_on(seg, rows, dev, who)
    H = _floor_metres(H, "H (the contact height)", who, zero_ok=False)
    hip.call("floor_stats", lo, ldl, tgt, ldt, ground, contact, seg, rows, H, out)
    return out


def floor_clamp(src, ground, seg, margin, dst, lifted=None, fallback=None):
    """dst[:, :24] = the lower-joint rows src [rows, >= 24] with every leg raised whose foot or ankle lies under ``margin`` metres above
    the row's plane (mmego_floor_clamp; the two-bone solve is in the header): bone lengths and the foot bone's vector are kept, hips
    and legs above the floor keep their bits, rows with seg < 0 too.  dst is src itself or shares no byte with it.  lifted [rows] fp32
    (optional): the larger lift of the two legs; fallback [rows] int32 (optional): the legs that fell back.  Everything is checked on
    the host first (ValueError)."""
    who = "floor_clamp"
    lds = _floor_rows(src, "src", None, 24, None, who)
    rows, dev = src.shape[0], src.device
    ldd = _floor_rows(dst, "dst", rows, 24, dev, who)
    _floor_rows(ground, "ground", rows, 4, dev, who, packed=True)
    seg = _seg_on(seg, rows, dev, who)
    margin = _floor_metres(margin, "margin", who, zero_ok=True)
    same = src.data_ptr() == dst.data_ptr() and lds == ldd
    if not same and _rows_overlap(src, lds, dst, ldd, rows, 24):
        raise ValueError("%s: dst overlaps src without being it" % who)
    _per_row(lifted, "lifted", rows, torch.float32, dev, who)
    _per_row(fallback, "fallback", rows, torch.int32, dev, who)
    hip.call("floor_clamp", src, lds, ground, seg, rows, margin, dst, ldd, lifted, fallback)
    return dst


RENDER_REC, RENDER_FIXED, RENDER_MAX_P = 12, 134, 1024        # render_math.h RD_REC, RD_FIXED, RD_MAX_P
# (cos, sin)(2 pi k / 32) of the floor ring's 32 vertices, float64 rounded once: the table mmego_render_prims is handed
RENDER_RING = np.stack([np.cos(2.0 * np.pi * np.arange(32) / 32.0), np.sin(2.0 * np.pi * np.arange(32) / 32.0)], axis=1).astype(np.float32)


def render_prims(pred, tgt, ground, cloud, seg, cam, vmax, prims):
    """prims [F, 134 + N, 12] = every frame's scene as 2-D primitives in layer order (mmego_render_prims; the layers are in the header):
    pred and tgt [F, >= 63] the predicted and the recorded joints, ground [F, 4] the planes, cloud [F, N, 6] the radar returns (N in
    [0, 890]), seg [F] int32 (a host array or a device tensor; < 0: the frame shows the target alone), cam [F, 8] the 2 x 4 affine of
    every frame, vmax > 0 the Doppler velocity at which the cloud's colour saturates.  Everything is checked on the host first (ValueError)."""
    who = "render_prims"
    ldp = _floor_rows(pred, "pred", None, 63, None, who)
    F, dev = pred.shape[0], pred.device
    ldt = _floor_rows(tgt, "tgt", F, 63, dev, who)
    _floor_rows(ground, "ground", F, 4, dev, who, packed=True)
    _floor_rows(cam, "cam", F, 8, dev, who, packed=True)
    if F >= 2 ** 31:
        raise ValueError("%s: %d frames do not fit the launch" % (who, F))
    if not (isinstance(cloud, torch.Tensor) and cloud.is_cuda and cloud.dtype == torch.float32 and cloud.dim() == 3 and cloud.device == dev
            and cloud.shape[0] == F and cloud.shape[2] == 6 and cloud.is_contiguous()):
        raise ValueError("%s: cloud is a contiguous fp32 tensor [%d, N, 6] on the rows' device" % (who, F))
    N = cloud.shape[1]
    if not 0 <= N <= RENDER_MAX_P - RENDER_FIXED:
        raise ValueError("%s: N = %d returns per frame lie outside [0, %d]" % (who, N, RENDER_MAX_P - RENDER_FIXED))
    seg = _seg_on(seg, F, dev, who)
    if isinstance(vmax, bool) or not isinstance(vmax, (int, float, np.integer, np.floating)) or not np.isfinite(vmax) or not vmax > 0:
        raise ValueError("%s: vmax is a finite velocity > 0, got %r" % (who, vmax))
    if not (isinstance(prims, torch.Tensor) and prims.is_cuda and prims.dtype == torch.float32 and prims.device == dev and prims.is_contiguous()
            and tuple(prims.shape) == (F, RENDER_FIXED + N, RENDER_REC) and prims.data_ptr() % 16 == 0):
        raise ValueError("%s: prims is a contiguous fp32 tensor [%d, %d, %d] on the rows' device, 16-byte aligned"
                         % (who, F, RENDER_FIXED + N, RENDER_REC))
    hip.call("render_prims", pred, ldp, tgt, ldt, ground, cloud if N else None, N, seg, cam, _upload_once(dev, RENDER_RING)[0], F, float(vmax),
             prims)
    return prims


def render_raster(prims, out, bg=(255, 255, 255)):
    """out [I, H, W, 3] (uint8) = the tables prims [I, P, 12] composited in index order over the background ``bg`` (mmego_render_raster;
    the recipe is in the header).  out may be a VIEW of a larger frame -- unit stride along the channels, 3 along x, a row pitch and an
    image stride that are multiples of 4 bytes -- so that two views share one frame; the bytes outside the view stay.  P in [0, 1024],
    W and H in [16, 2048], W a multiple of 4.  Everything is checked on the host first (ValueError)."""
    who = "render_raster"
    if not (isinstance(prims, torch.Tensor) and prims.is_cuda and prims.dtype == torch.float32 and prims.dim() == 3):
        raise ValueError("%s: prims is a 3-D fp32 device tensor" % who)
    I, P = prims.shape[0], prims.shape[1]
    if I < 1 or not 0 <= P <= RENDER_MAX_P or prims.shape[2] != RENDER_REC or not prims.is_contiguous():
        raise ValueError("%s: prims is %s, wanted contiguous [I >= 1, P in [0, %d], %d]" % (who, tuple(prims.shape), RENDER_MAX_P, RENDER_REC))
    if prims.data_ptr() % 16:
        raise ValueError("%s: prims is not 16-byte aligned" % who)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.dim() == 4 and out.device == prims.device):
        raise ValueError("%s: out is a 4-D uint8 tensor on the primitives' device" % who)
    if out.shape[0] != I or out.shape[3] != 3:
        raise ValueError("%s: out is %s for %d images of 3-byte pixels" % (who, tuple(out.shape), I))
    H, W = out.shape[1], out.shape[2]
    if not (16 <= W <= 2048 and 16 <= H <= 2048) or W % 4:
        raise ValueError("%s: W = %d and H = %d have to lie in [16, 2048], W a multiple of 4" % (who, W, H))
    stride, pitch = out.stride(0) if I > 1 else max(out.stride(0), H * out.stride(1)), out.stride(1)
    if out.stride(3) != 1 or out.stride(2) != 3:
        raise ValueError("%s: out's pixels are 3 adjacent bytes, a row's pixels adjacent, got strides %s" % (who, tuple(out.stride())))
    if pitch < 3 * W or pitch % 4:
        raise ValueError("%s: the row pitch %d is below 3 W = %d or no multiple of 4" % (who, pitch, 3 * W))
    if stride < H * pitch or stride % 4:
        raise ValueError("%s: the image stride %d is below H x pitch = %d or no multiple of 4" % (who, stride, H * pitch))
    if out.data_ptr() % 4:
        raise ValueError("%s: out is not 4-byte aligned" % who)
    if I * ((W + 31) // 32) * ((H + 31) // 32) >= 2 ** 31:
        raise ValueError("%s: %d images of %d x %d pixels do not fit one launch" % (who, I, W, H))
    if not (isinstance(bg, (tuple, list)) and len(bg) == 3
            and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v <= 255 for v in bg)):
        raise ValueError("%s: bg is three integer levels in [0, 255], got %r" % (who, bg))
    if P == 0:                                                     # (an empty tensor has no address; the ABI refuses a null pointer)
        prims = _upload_once(prims.device, np.zeros((1, RENDER_REC), dtype=np.float32))[0]
    hip.call("render_raster", prims, I, P, out, W, H, pitch, stride, int(bg[0]), int(bg[1]), int(bg[2]))
    return out


def fill(t, v):
    if not t.is_contiguous():
        raise ValueError("fill needs a contiguous tensor")
    hip.call("fill", t, t.numel(), float(v))
    return t


def copy2d(X, Y, accumulate=False):
    X, Y = _rows(X), _rows(Y)
    if X.shape != Y.shape:
        raise ValueError("copy2d shape mismatch")
    hip.call("copy2d", X, X.stride(0), Y, Y.stride(0), X.shape[0], X.shape[1], int(accumulate))
    return Y


def seed_take(seed_ctr, taken):
    """taken[0] = seed_ctr[0]; seed_ctr[0] advances as mmego_inc_i64 advances it (int64 device words)."""
    for t in (seed_ctr, taken):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.numel() >= 1):
            raise TypeError("seed_take needs int64 device words")
    hip.call("seed_take", seed_ctr, taken)
    return taken


def lstm_dropout(x, y, p, seed_word, salt):
    """y = x * mask: nn.LSTM(dropout=p)'s inverted dropout from the counter-based hash of (logical element index, seed_word[0], salt)
    (mmego_lstm_dropout; the kernel refuses p outside (0, 1) and a column count that is no multiple of 4).  y may be x."""
    x, y = _rows(x), _rows(y)
    if x.shape != y.shape:
        raise ValueError("lstm_dropout shape mismatch")
    if not (isinstance(seed_word, torch.Tensor) and seed_word.is_cuda and seed_word.dtype == torch.int64):
        raise TypeError("lstm_dropout needs an int64 device seed word")
    hip.call("lstm_dropout", x, x.stride(0), y, y.stride(0), x.shape[0], x.shape[1], float(p), seed_word, int(salt))
    return y


def gather_rows(X, idx, Y):
    """Y[i, :] = X[idx[i], :] for contiguous fp32 X [n, W], int64 idx [m], Y [m, W]."""
    _chk(X, 2), _chk(Y, 2)
    if not (X.is_contiguous() and Y.is_contiguous() and idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous()):
        raise ValueError("gather_rows needs contiguous fp32 X/Y and a contiguous int64 device index")
    if Y.shape != (idx.numel(), X.shape[1]):
        raise ValueError("gather_rows shape mismatch")
    hip.call("gather_rows", X, X.shape[0], X.shape[1], idx, idx.numel(), Y)
    return Y


PACK_FRAMES_MAX_PC_NO = 1024


def pack_frames_max_n(pc_no):
    """The largest per-frame point count mmego_pack_frames takes at ``pc_no`` slots: 64 KB of LDS, four waves, per wave
    max(max_n, pc_no) keys and max_n survivor numbers."""
    words = 64 * 1024 // 4 // 4
    return max(0, min(words // 2, words - int(pc_no)))


def _pack_frames_check(pts, frame_off, frame_idx, out):
    _chk(pts, 2)
    if not (pts.is_contiguous() and pts.shape[1] == 5 and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
            and out.dim() == 3 and out.shape[2] == 6):
        raise ValueError("pack_frames needs contiguous fp32 points [P, 5] and a contiguous fp32 out [nout, pc_no, 6]")
    for t in (frame_off, frame_idx):
        if not (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.dim() == 1):
            raise ValueError("pack_frames needs contiguous int64 device offsets and frame numbers")
    if frame_idx.numel() != out.shape[0] or frame_off.numel() < 2:
        raise ValueError("pack_frames shape mismatch")


def pack_frames(pts, frame_off, frame_idx, out, max_n, keep_p, seed):
    """out[q] [pc_no, 6] = a fresh random packing of the raw points [P, 5] of frame frame_idx[q] (int64 CSR offsets frame_off; every
    index has to lie in [0, len(frame_off) - 1): the caller's to check, the index lives on the device), each point kept with probability
    keep_p (mmego_pack_frames: the recipe is in the header).  The same ``seed`` (an integer below 2^64) gives the same output."""
    _pack_frames_check(pts, frame_off, frame_idx, out)
    hip.call("pack_frames", pts, frame_off, frame_idx, frame_idx.numel(), out.shape[1], int(max_n), float(keep_p),
             int(seed) & 0xFFFFFFFFFFFFFFFF, out)
    return out


def pack_frames_noise(pts, frame_off, frame_idx, out, max_n, keep_p, seed, sigma_xyz, sigma_v):
    """pack_frames -- the same returns in the same slots for the same ``seed`` and ``keep_p`` -- with every kept return perturbed before
    its row is written: x, y, z by sigma_xyz z and the velocity by sigma_v z, z a centred sum of four uniforms of unit variance and
    support +-2 sqrt(3) drawn per (seed, output frame, return, channel); r is formed from the perturbed x, y, z and the intensity is
    copied (mmego_pack_frames_noise: the recipe is in the header).  A sigma of 0 leaves its channels' bits alone."""
    _pack_frames_check(pts, frame_off, frame_idx, out)
    hip.call("pack_frames_noise", pts, frame_off, frame_idx, frame_idx.numel(), out.shape[1], int(max_n), float(keep_p),
             int(seed) & 0xFFFFFFFFFFFFFFFF, float(sigma_xyz), float(sigma_v), out)
    return out


def pose_jitter(R, t, sigma_deg, sigma_t, word, R_out, t_out, ids=None):
    """(R_out, t_out) = the head poses R [..., 3, 3], t [..., 3] each perturbed by a random rotation (rotation vector of standard
    deviation sigma_deg degrees per axis, never beyond 6 sigma_deg in all) and a random shift (sigma_t per component, never beyond
    3.47 sigma_t), drawn from ``word`` -- ONE int64 word on the device, read by the kernel, so a captured launch draws afresh once the
    word is rewritten -- and the row's draw number: ids[i] (int64 on the device, one per row) or the row number (mmego_pose_jitter: the
    recipe is in the header).  A sigma of 0 copies its half bit for bit; both 0 are refused.  R_out may be R and t_out may be t."""
    for x, tail, what in ((R, (3, 3), "R"), (t, (3,), "t"), (R_out, (3, 3), "R_out"), (t_out, (3,), "t_out")):
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape[-len(tail):]) == tail
                and x.dim() > len(tail)):
            raise ValueError("pose_jitter: %s is a contiguous fp32 tensor [..., %s]" % (what, ", ".join(map(str, tail))))
    n = R.numel() // 9
    if n < 1 or t.numel() != 3 * n or R_out.numel() != 9 * n or t_out.numel() != 3 * n:
        raise ValueError("pose_jitter: R %s, t %s, R_out %s and t_out %s do not hold one and the same number of poses"
                         % tuple(tuple(x.shape) for x in (R, t, R_out, t_out)))
    if not (isinstance(word, torch.Tensor) and word.dtype == torch.int64 and word.numel() >= 1 and word.is_contiguous()
            and word.device.type == "cuda"):
        raise TypeError("pose_jitter needs an int64 device seed word")
    if ids is not None:
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int64 and ids.is_contiguous() and ids.device.type == "cuda"):
            raise TypeError("pose_jitter: ids are contiguous int64 draw numbers on the device")
        if ids.numel() != n:
            raise ValueError("pose_jitter: %d ids for %d poses" % (ids.numel(), n))
    for x in (R, t, R_out, t_out):
        _chk(x, x.dim())
    hip.call("pose_jitter", R, t, n, float(sigma_deg), float(sigma_t), word, ids, R_out, t_out)
    return R_out, t_out


def imu_jitter(imu, sigmas, word, out, T=None, row_ids=None, win_ids=None):
    """out = the IMU samples imu [..., T, S, 15] (orientation 3 x 3, accelerometer, gyroscope) perturbed by white noise per sample and a
    bias that is constant over a window of T frames.  ``sigmas`` = (noise_rot_deg, noise_acc, noise_gyro, bias_rot_deg, bias_acc,
    bias_gyro): degrees per axis of the rotation vector, the additive ones in the recordings' units.  The draws come from ``word`` --
    ONE int64 word on the device, read by the kernel, so a captured launch draws afresh once the word is rewritten -- and the draw
    numbers: row_ids (int64 on the device, one per frame) or the frame's number, win_ids (one per window) or the window's number
    (mmego_imu_jitter: the recipe is in the header).  T None: the third dimension from the end; T given: imu is [..., S, 15] and its
    frames fall into windows of T.  A group both of whose sigmas are 0 is copied bit for bit; all six 0 are refused.  out may be imu.
    -> out."""
    for x, what in ((imu, "imu"), (out, "out")):
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 3 and x.shape[-1] == 15):
            raise ValueError("imu_jitter: %s is a contiguous fp32 tensor [..., T, S, 15]" % what)
    if tuple(out.shape) != tuple(imu.shape):
        raise ValueError("imu_jitter: imu %s and out %s differ in shape" % (tuple(imu.shape), tuple(out.shape)))
    S = int(imu.shape[-2])
    n = imu.numel() // (15 * S) if S else 0
    T = int(imu.shape[-3]) if T is None else int(T)
    if n < 1 or T < 1 or n % T:
        raise ValueError("imu_jitter: imu %s does not hold whole windows of T = %d frames" % (tuple(imu.shape), T))
    sig = tuple(float(v) for v in sigmas)
    if len(sig) != 6 or not all(0.0 <= v < float("inf") for v in sig) or not any(sig):
        raise ValueError("imu_jitter: sigmas are six finite values >= 0, one of them > 0, got %r" % (tuple(sigmas),))
    if not (isinstance(word, torch.Tensor) and word.dtype == torch.int64 and word.numel() >= 1 and word.is_contiguous()
            and word.device.type == "cuda"):
        raise TypeError("imu_jitter needs an int64 device seed word")
    for ids, want, what in ((row_ids, n, "row_ids"), (win_ids, n // T, "win_ids")):
        if ids is None:
            continue
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int64 and ids.is_contiguous() and ids.device.type == "cuda"):
            raise TypeError("imu_jitter: %s are contiguous int64 draw numbers on the device" % what)
        if ids.numel() != want:
            raise ValueError("imu_jitter: %d %s for %d %s" % (ids.numel(), what, want, "frames" if what == "row_ids" else "windows"))
    for x in (imu, out):
        _chk(x, x.dim())
    hip.call("imu_jitter", imu, n, T, S, *sig, word, row_ids, win_ids, out)
    return out


def relu_mask_(G, H):
    G, H = _rows(G), _rows(H)
    hip.call("relu_mask", G, G.stride(0), H, H.stride(0), G.shape[0], G.shape[1])
    return G


class BnState:
    """mean / invstd / a / b vectors of one BatchNorm application (kept for backward)."""

    def __init__(self, arena, key, C):
        v = arena.get(key, (4, C))
        self.all = v
        self.mean, self.invstd, self.a, self.b = v[0], v[1], v[2], v[3]
        self.C = C


def bn_stats(arena, key, X, bn, training):
    """Compute the affine of a BatchNorm over the rows of X (train: batch stats + running update)."""
    X = _rows(X)
    rows, C = X.shape
    st = BnState(arena, key, C)
    if training:
        ws = scratch(X.device, 3 * C * hip.colstats_nblk(rows))
        hip.call("bn_train_stats", X, X.stride(0), rows, C, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                 float(bn.momentum), float(bn.eps), ws, st.mean, st.invstd, st.a, st.b)
        # num_batches_tracked is bumped once per forward for the whole net (FlatParams.tick_args)
    else:
        hip.call("bn_eval_affine", C, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps),
                 st.mean, st.invstd, st.a, st.b)
    return st


def bn_stats_pair(arena, key1, X1, bn1, key2, X2, bn2, training):
    """bn_stats of two same-shape tensors; in training one pair of launches instead of two (same results)."""
    X1, X2 = _rows(X1), _rows(X2)
    rows, C = X1.shape
    tc = 8
    while tc < C and tc < 64:
        tc <<= 1
    if not training or X2.shape != X1.shape or C % tc:
        return bn_stats(arena, key1, X1, bn1, training), bn_stats(arena, key2, X2, bn2, training)
    st1, st2 = BnState(arena, key1, C), BnState(arena, key2, C)
    ws = scratch(X1.device, 6 * C * hip.colstats_nblk(rows))
    hip.call("bn_train_stats_pair", rows, C, ws,
             X1, X1.stride(0), bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, float(bn1.momentum), float(bn1.eps),
             st1.mean, st1.invstd, st1.a, st1.b,
             X2, X2.stride(0), bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var, float(bn2.momentum), float(bn2.eps),
             st2.mean, st2.invstd, st2.a, st2.b)
    return st1, st2


def affine_act(X, st, Y, relu=True, X2=None, st2=None):
    X, Y = _rows(X), _rows(Y)
    rows, C = X.shape
    if X2 is not None:
        X2 = _rows(X2)
        hip.call("affine_act", X, X.stride(0), st.mean, st.a, st.b, X2, X2.stride(0), st2.mean, st2.a, st2.b, Y,
                 Y.stride(0), rows, C, int(relu))
    else:
        hip.call("affine_act", X, X.stride(0), st.mean, st.a, st.b, None, 0, None, None, None, Y, Y.stride(0), rows, C,
                 int(relu))
    return Y


def bn_backward(dY, Ymask, X, st, dgamma, dbeta, dX):
    """BatchNorm(train) backward through an optional ReLU (mask = Ymask > 0)."""
    dY, X, dX = _rows(dY), _rows(X), _rows(dX)
    rows, C = X.shape
    ws = scratch(X.device, 2 * C * hip.colstats_nblk(rows) + 2 * C)
    c12 = ws[2 * C * hip.colstats_nblk(rows):]
    if Ymask is not None:
        Ymask = _rows(Ymask)
        hip.call("bn_backward", dY, dY.stride(0), Ymask, Ymask.stride(0), X, X.stride(0), st.mean, st.invstd, st.a, rows,
                 C, ws, c12, dgamma, dbeta, dX, dX.stride(0))
    else:
        hip.call("bn_backward", dY, dY.stride(0), None, 0, X, X.stride(0), st.mean, st.invstd, st.a, rows, C, ws, c12,
                 dgamma, dbeta, dX, dX.stride(0))
    return dX


def bn_backward_pair(dY, Ymask, X1, st1, dgamma1, dbeta1, dX1, X2, st2, dgamma2, dbeta2, dX2):
    """Two BatchNorm(train) backwards that share dY and the ReLU mask, in the launches of one (same bits as two bn_backward calls)."""
    dY, Ymask, X1, dX1, X2, dX2 = (_rows(t) for t in (dY, Ymask, X1, dX1, X2, dX2))
    rows, C = X1.shape
    tc = 8
    while tc < C and tc < 64:
        tc <<= 1
    if X2.shape != X1.shape or C % tc:
        bn_backward(dY, Ymask, X1, st1, dgamma1, dbeta1, dX1)
        bn_backward(dY, Ymask, X2, st2, dgamma2, dbeta2, dX2)
        return
    nblk = hip.colstats_nblk(rows)
    ws = scratch(X1.device, 4 * C * nblk + 4 * C)
    hip.call("bn_backward_pair", dY, dY.stride(0), Ymask, Ymask.stride(0), rows, C, ws, ws[4 * C * nblk:],
             X1, X1.stride(0), st1.mean, st1.invstd, st1.a, dgamma1, dbeta1, dX1, dX1.stride(0),
             X2, X2.stride(0), st2.mean, st2.invstd, st2.a, dgamma2, dbeta2, dX2, dX2.stride(0))


def transform2h_(pts, R, t, src=None, keep=None, feats=None, nfeat=0):
    """In place on pts [F, P, C] (or any contiguous view of it).  src (optional): the points are read from there -- [F, P, 3]
    (xyz only) or a tensor of pts' shape (whole rows: the other channels are copied along).  keep (optional, pts' shape) and
    feats (optional 2-D [F*P, >= nfeat] view with unit column stride: its first nfeat columns) receive the transformed rows too."""
    _chk(pts)
    if not pts.is_contiguous():
        raise ValueError("transform2h_ needs a contiguous point tensor")
    F = R.numel() // 9
    C = pts.shape[-1]
    P = pts.numel() // (F * C)
    src_ld = 0
    if src is not None:
        if not (src.is_contiguous() and src.dtype == torch.float32):
            raise ValueError("transform2h_: src must be a contiguous fp32 tensor")
        if src.numel() * C == 3 * pts.numel():
            src_ld = 3
        elif src.numel() == pts.numel():
            src_ld = C
        else:
            raise ValueError("transform2h_: src must hold one xyz row or one whole row per point")
    if keep is not None and not (keep.is_contiguous() and keep.dtype == torch.float32 and keep.numel() == pts.numel()):
        raise ValueError("transform2h_: keep must be a contiguous fp32 tensor of pts' size")
    ldf = 0
    if feats is not None:
        if not (feats.dim() == 2 and feats.stride(1) == 1 and feats.shape[0] * C == pts.numel() and 1 <= nfeat <= min(C, feats.shape[1])):
            raise ValueError("transform2h_: feats must be a [points, >= nfeat] view with unit column stride")
        ldf = feats.stride(0)
    if not (R.is_contiguous() and t.is_contiguous() and t.numel() == 3 * F):
        raise ValueError("R/t must be contiguous [F,3,3]/[F,3]")
    hip.call("transform2h", pts, F, P, C, R, t, src, src_ld, keep, feats, ldf, nfeat)
    return pts


def rotate_points(inp, out, R, t=None, transpose=True):
    F = R.numel() // 9
    P = inp.numel() // (3 * F)
    if not (inp.is_contiguous() and out.is_contiguous() and R.is_contiguous()):
        raise ValueError("rotate_points needs contiguous tensors")
    hip.call("rotate_points", inp, out, F, P, R, t, int(transpose), int(t is not None))
    return out
