"""GPU: the temporal filter of dense inference in its column form (csrc/smooth.hip, mmego_smooth_frames) against the float64 restatement
of tests/smooth_ref.py -- whose coefficients come from a least-squares solve, not from the kernel's cofactors -- on N(0, 0.7) rows.

Bound: |out - ref| <= 2^-23 |ref| + 1e-7 on every element of dst and moved (dense_ref.within <= 1, the bound of the double-inside,
float-store kernels).  Worked out on the CPU (scripts/smooth_host_check.hip, the kernel's arithmetic lane by lane against long-double
sums): the coefficients of the two routes agree to 1.5e-14, sum |c_k| <= 2.5, the stored output comes to 0.41 of the bound.

The segment layout: a segment of one frame (its row bit for bit, moved 0), one of two (the degree falls to 1), an uncovered frame (-1: its
row bit for bit), a segment that ends at frame 63 and one that starts at frame 64 (the edge of a wave's workgroup), another gap, the rest;
at F = 3 also one segment over the three frames, whose windows overhang both ends of the array for every H."""
import numpy as np
import pytest
import torch

import dense_ref as ref
import smooth_ref as sref

pytestmark = pytest.mark.gpu

SENT = -12345.0
HS, DS, TABLES = (1, 3, 31), (0, 1, 2), ("box", "gauss", "random")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _d(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def layout(F, whole=False):
    seg = np.repeat([5, 2, -1, 7, 1, -1, 3], [1, 2, 1, 60, 100, 2, 400]).astype(np.int32)[:F]
    return np.zeros(F, np.int32) if whole else seg


def table(rng, H, kind):
    return sref.weights(H, kind) if kind != "random" else rng.uniform(0.5, 2.0, 2 * H + 1).astype(np.float32)


def _raw(dev, src, seg, w, D, pad_s=0, pad_d=0, moved=True):
    """The entry point itself on a source of row stride C + pad_s and a dst of row stride C + pad_d with one more row behind the last."""
    from mmego_amd import hip
    F, C = src.shape
    wide = np.full((F, C + pad_s), 777.0, np.float32)
    wide[:, :C] = src
    dst = torch.full((F + 1, C + pad_d), SENT, dtype=torch.float32, device=dev)
    mv = torch.full((F + 1,), SENT, dtype=torch.float32, device=dev)
    hip.call("smooth_frames", _d(dev, wide), C + pad_s, F, C, _d(dev, seg), _d(dev, w), len(w) // 2, D, dst, C + pad_d,
             mv if moved else None)
    return dst, mv


@pytest.mark.parametrize("C", [24, 45, 63, 64])
@pytest.mark.parametrize("F", [1, 3, 64, 65, 257])
def test_smooth_frames_against_the_restatement(dev, F, C):
    rng = np.random.default_rng(1000 * F + C)
    src = rng.normal(0.0, 0.7, (F, C)).astype(np.float32)
    worst, worst_m, case = 0.0, 0.0, 0
    for whole in ((False, True) if F == 3 else (False,)):
        seg = layout(F, whole)
        for H in HS:
            for D in DS:
                for kind in TABLES:
                    w = table(rng, H, kind)
                    want, want_m = sref.smooth_frames(src, seg, w, D)
                    case += 1
                    pad_s, pad_d = (0, 0) if case % 2 else (3, 5)
                    with_moved = C % 3 == 0
                    dst, mv = _raw(dev, src, seg, w, D, pad_s, pad_d, with_moved)
                    out, m = dst.cpu().numpy(), mv.cpu().numpy()
                    assert np.all(out[:F, C:] == SENT) and np.all(out[F] == SENT) and m[F] == SENT, "written outside the F rows of C columns"
                    assert not np.isnan(out).any()
                    worst = max(worst, ref.within(out[:F, :C], want))
                    # rows outside every segment, or alone in their own: bit for bit
                    alone = np.asarray([len(sref.valid_taps(seg, f, H)) <= 1 for f in range(F)])
                    assert np.array_equal(out[:F, :C][alone], src[alone]), (H, D, kind)
                    if with_moved:
                        worst_m = max(worst_m, ref.within(m[:F], want_m))
                        assert not m[:F][alone].any()
                    else:
                        assert (m == SENT).all()
                    dst2, mv2 = _raw(dev, src, seg, w, D, pad_s, pad_d, with_moved)
                    assert torch.equal(dst, dst2) and torch.equal(mv, mv2), "two launches, the same bits"
        if not whole:
            n_alone = int(np.sum([len(sref.valid_taps(seg, f, 1)) <= 1 for f in range(F)]))
            assert n_alone >= (1 if F <= 3 else 2)
    print("F %d C %d: worst error / bound %.3f (dst) %.3f (moved) over %d launches" % (F, C, worst, worst_m, case))
    assert worst <= 1.0 and worst_m <= 1.0


@pytest.mark.parametrize("D", DS)
def test_polynomials_of_degree_D_come_back(dev, D):
    """Rows that are polynomials of degree <= D in the frame number with small integer coefficients -- exact as float32 -- come back
    within the bound, at segment edges and array ends too (where fewer than D + 1 taps are valid the fit of degree n - 1 interpolates
    its n points, so the frame's own value comes back there as well); so do constant rows for every D."""
    rng = np.random.default_rng(D)
    F, C = 257, 45
    seg = layout(F)
    t = np.arange(F, dtype=np.float64)[:, None] - 128.0
    coef = [rng.integers(-100, 101, C), rng.integers(-20, 21, C), rng.integers(-3, 4, C)]
    x = sum(coef[m].astype(np.float64) * t ** m for m in range(D + 1))
    const = np.tile(rng.normal(0, 0.7, C).astype(np.float32), (F, 1)).astype(np.float64)
    for rows in (x, const):
        assert np.array_equal(rows.astype(np.float32).astype(np.float64), rows)
        for H in HS:
            for kind in TABLES:
                dst, _ = _raw(dev, rows.astype(np.float32), seg, table(rng, H, kind), D)
                worst = ref.within(dst.cpu().numpy()[:F], rows)
                assert worst <= 1.0, (H, kind, worst)


def test_a_segment_does_not_see_its_neighbours(dev):
    rng = np.random.default_rng(9)
    F, C = 257, 63
    seg = layout(F)
    src = rng.normal(0.0, 0.7, (F, C)).astype(np.float32)
    other = src.copy()
    mine = seg == 1                                      # frames 64 .. 163
    other[~mine] = rng.normal(0.0, 50.0, (int((~mine).sum()), C)).astype(np.float32)
    for H, D in ((31, 2), (3, 1), (1, 0)):
        w = table(rng, H, "gauss")
        a, ma = _raw(dev, src, seg, w, D)
        b, mb = _raw(dev, other, seg, w, D)
        assert torch.equal(a[:F][_d(dev, mine)], b[:F][_d(dev, mine)]) and torch.equal(ma[:F][_d(dev, mine)], mb[:F][_d(dev, mine)])
        assert not torch.equal(a, b)


def test_refusals_leave_the_outputs_alone(dev):
    from mmego_amd import dense, hip, ops
    rng = np.random.default_rng(3)
    F, C = 20, 45
    src = _d(dev, rng.normal(0.0, 0.7, (F, C)).astype(np.float32))
    seg = np.zeros(F, np.int32)
    w = dense.smooth_weights(3, "gauss")
    dst = torch.full((F, C), SENT, dtype=torch.float32, device=dev)
    mv = torch.full((F,), SENT, dtype=torch.float32, device=dev)
    both = torch.full((2 * F, C), SENT, dtype=torch.float32, device=dev)
    zero, nan, inf = w.copy(), w.copy(), w.copy()
    zero[2], nan[4], inf[0] = 0.0, np.nan, np.inf
    for what, call in (("dst is src", lambda: ops.smooth_frames(src, seg, w, 2, src, mv)),
                       ("dst overlaps src", lambda: ops.smooth_frames(both[:F], seg, w, 2, both[F - 1:2 * F - 1], mv)),
                       ("an even weight length", lambda: ops.smooth_frames(src, seg, w[:-1], 2, dst, mv)),
                       ("H = 32", lambda: ops.smooth_frames(src, seg, np.ones(65, np.float32), 2, dst, mv)),
                       ("H = 0", lambda: ops.smooth_frames(src, seg, np.ones(1, np.float32), 2, dst, mv)),
                       ("a zero weight", lambda: ops.smooth_frames(src, seg, zero, 2, dst, mv)),
                       ("a NaN weight", lambda: ops.smooth_frames(src, seg, nan, 2, dst, mv)),
                       ("an infinite weight", lambda: ops.smooth_frames(src, seg, inf, 2, dst, mv)),
                       ("a negative weight", lambda: ops.smooth_frames(src, seg, -w, 2, dst, mv)),
                       ("order 3", lambda: ops.smooth_frames(src, seg, w, 3, dst, mv)),
                       ("order -1", lambda: ops.smooth_frames(src, seg, w, -1, dst, mv)),
                       ("a short seg", lambda: ops.smooth_frames(src, seg[:-1], w, 2, dst, mv)),
                       ("an int64 seg", lambda: ops.smooth_frames(src, seg.astype(np.int64), w, 2, dst, mv)),
                       ("an int64 device seg", lambda: ops.smooth_frames(src, _d(dev, seg.astype(np.int64)), w, 2, dst, mv)),
                       ("a short dst", lambda: ops.smooth_frames(src, seg, w, 2, dst[:, :44], mv)),
                       ("a dst of other frames", lambda: ops.smooth_frames(src, seg, w, 2, dst[:F - 1], mv)),
                       ("moved of other frames", lambda: ops.smooth_frames(src, seg, w, 2, dst, mv[:F - 1])),
                       ("moved for rows that are no 3-vectors", lambda: ops.smooth_frames(src[:, :44], seg, w, 2, dst, mv)),
                       ("65 columns", lambda: ops.smooth_frames(torch.zeros((F, 65), device=dev), seg, w, 2, torch.zeros((F, 65), device=dev)))):
        with pytest.raises(ValueError):
            call()
        torch.cuda.synchronize()
        assert bool((dst == SENT).all()) and bool((mv == SENT).all()) and bool((both == SENT).all()), what
    # the entry point itself
    segd, wd = _d(dev, seg), _d(dev, w)
    good = dict(src=src, lds=C, F=F, C=C, seg=segd, w=wd, H=3, D=2, dst=dst, ldd=C, moved=mv)
    for change in (dict(src=None), dict(seg=None), dict(w=None), dict(dst=None), dict(F=0), dict(C=0), dict(C=65, lds=65, ldd=65),
                   dict(lds=44), dict(ldd=44), dict(H=0), dict(H=32), dict(D=-1), dict(D=3), dict(C=44, moved=mv), dict(dst=src)):
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("smooth_frames", *[a[k] for k in good])
    torch.cuda.synchronize()
    assert bool((dst == SENT).all()) and bool((mv == SENT).all())
    ops.smooth_frames(src, seg, w, 2, dst, mv)                          # (and the good call goes through, with a device seg as well)
    again = torch.full((F, C), SENT, dtype=torch.float32, device=dev)
    ops.smooth_frames(src, segd, w, 2, again)
    assert not bool((dst == SENT).any()) and not bool((mv == SENT).any()) and torch.equal(dst, again)
