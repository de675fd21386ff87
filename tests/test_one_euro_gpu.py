"""GPU: dense inference's causal filter alone (csrc/one_euro.hip: mmego_one_euro, mmego_one_euro_bones) against the float64 restatement
of tests/one_euro_ref.py, on N(0, 0.7) rows (column form) and on slowly moving rigid skeletons over the walk tables of skeleton.py
(bones form).

Bound: |out - ref| <= 2^-23 |ref| + 1e-7 on every element of dst and moved (dense_ref.within <= 1), the bound tests/test_smooth_gpu.py
holds mmego_smooth_frames to: double inside, one float store.  Worked out on the CPU (scripts/one_euro_host_check.hip, the kernels'
arithmetic step by step against a long-double recursion): the stored output comes to 0.40 of the bound, a filtered bone to 9.4e-8 m of
its length, and a bone that reverses every frame at alpha = 1/2 cancels in the run's second frame and in no other.

The layout, F = 150: copy runs (uncovered stretches) of 2 frames at the head, 5 in the middle and 12 at the tail; filter runs of 1, 2,
3, 65 and 60 frames -- 65 is longer than a wave and than the kernel's read-ahead ring (8 frames), 1, 2 and 3 end inside it."""
import numpy as np
import pytest
import torch

import dense_ref as ref
import one_euro_ref as oref

pytestmark = pytest.mark.gpu

SENT = -12345.0
RIGID = 2e-6
SEG = np.repeat([-1, 5, 2, -1, 7, 1, 3, -1], [2, 1, 2, 5, 3, 65, 60, 12]).astype(np.int32)
F = len(SEG)
PARAMS = [(fc, beta) for fc in (0.02, 5.0) for beta in (0.0, 40.0)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _d(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _trees():
    from mmego_amd import skeleton
    return {"upper": (15, np.asarray(skeleton.WALK_UPPER, np.int32)), "lower": (8, np.asarray(skeleton.WALK_LOWER, np.int32))}


def _raw(dev, src, runs, fc, beta, dc, pad_s=0, pad_d=0, moved=True, bones=None, L=None, fallback=True):
    """The entry point itself on a source of row stride C + pad_s and a dst of row stride C + pad_d with one more row behind the last."""
    from mmego_amd import hip
    rows, C = src.shape
    wide = np.full((rows, C + pad_s), 777.0, np.float32)
    wide[:, :C] = src
    dst = torch.full((rows + 1, C + pad_d), SENT, dtype=torch.float32, device=dev)
    mv = torch.full((rows + 1,), SENT, dtype=torch.float32, device=dev)
    fb = torch.full((rows + 1,), -7, dtype=torch.int32, device=dev)
    head = (_d(dev, wide), C + pad_s, rows, C // 3, _d(dev, runs[0]), _d(dev, runs[1]), len(runs[1]), fc, beta, dc)
    if bones is None:
        hip.call("one_euro", *head, dst, C + pad_d, mv if moved else None)
    else:
        hip.call("one_euro_bones", *head, _d(dev, np.asarray(bones, np.int32)), _d(dev, np.asarray(L, np.float32)), len(bones), dst,
                 C + pad_d, mv if moved else None, fb if fallback else None)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), mv.cpu().numpy(), fb.cpu().numpy()


def _untouched(out, mv, rows, C, fb=None):
    assert np.all(out[:rows, C:] == SENT) and np.all(out[rows] == SENT) and mv[rows] == SENT, "written outside the rows' 3 J columns"
    assert fb is None or fb[rows] == -7


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("J", [15, 8])
def test_one_euro_against_the_restatement(dev, J, pad):
    from mmego_amd import ops
    rng = np.random.default_rng(100 * J + pad)
    C = 3 * J
    src = rng.normal(0.0, 0.7, (F, C)).astype(np.float32)
    runs = ops.one_euro_runs(SEG)
    assert runs[0].tolist() == [0, 2, 3, 5, 10, 13, 78, 138, 150] and runs[1].tolist() == [0, 1, 1, 0, 1, 1, 1, 0]
    copied = np.repeat(runs[1] == 0, np.diff(runs[0]))
    firsts = runs[0][:-1]
    worst = worst_m = 0.0
    for fc, beta in PARAMS:
        want, want_m = oref.one_euro(src, runs, fc, beta, 0.1)
        out, mv, _ = _raw(dev, src, runs, fc, beta, 0.1, pad, pad)
        _untouched(out, mv, F, C)
        assert not np.isnan(out).any()
        worst, worst_m = max(worst, ref.within(out[:F, :C], want)), max(worst_m, ref.within(mv[:F], want_m))
        assert out[:F, :C][copied].tobytes() == src[copied].tobytes(), "the rows of copy runs, bit for bit"
        assert out[:F, :C][firsts].tobytes() == src[firsts].tobytes(), "the first row of every run, bit for bit"
        assert (mv[:F][copied] == 0.0).all() and (mv[:F][firsts] == 0.0).all()
        assert (out[:F, :C][~copied] != src[~copied]).mean() > 0.9, "the filter ran"
        # two launches, the same bits; without moved the same dst and that buffer untouched
        out2, mv2, _ = _raw(dev, src, runs, fc, beta, 0.1, pad, pad)
        assert out2.tobytes() == out.tobytes() and mv2.tobytes() == mv.tobytes()
        out3, mv3, _ = _raw(dev, src, runs, fc, beta, 0.1, pad, pad, moved=False)
        assert out3.tobytes() == out.tobytes() and (mv3 == SENT).all()
    print("one_euro J %d pad %d: dst worst error / bound %.3f, moved %.3f" % (J, pad, worst, worst_m))
    assert worst <= 1.0 and worst_m <= 1.0


@pytest.mark.parametrize("J", [15, 8])
def test_a_single_frame(dev, J):
    src = np.random.default_rng(J).normal(0.0, 0.7, (1, 3 * J)).astype(np.float32)
    for on in (1, 0):
        out, mv, _ = _raw(dev, src, (np.asarray([0, 1], np.int64), np.asarray([on], np.int32)), 0.05, 10.0, 0.1, 3, 5)
        _untouched(out, mv, 1, 3 * J)
        assert out[:1, :3 * J].tobytes() == src.tobytes() and mv[0] == 0.0


@pytest.mark.parametrize("fc,beta", PARAMS)
def test_what_holds_bit_for_bit(dev, fc, beta):
    """A constant run comes back exactly; a run does not see the other runs; a frame does not see the frames behind it."""
    from mmego_amd import ops
    rng = np.random.default_rng(17)
    J = 15
    src = rng.normal(0.0, 0.7, (F, 3 * J)).astype(np.float32)
    src[13:78] = src[13]                                                    # the 65-frame run: one row, 65 times
    runs = ops.one_euro_runs(SEG)
    out, mv, _ = _raw(dev, src, runs, fc, beta, 0.1)
    assert out[13:78, :45].tobytes() == src[13:78].tobytes() and (mv[13:78] == 0.0).all()
    other = src.copy()
    keep = np.zeros(F, bool)
    keep[78:138] = True                                                     # the 60-frame run stays, every other row changes
    other[~keep] = rng.normal(0.0, 0.7, ((~keep).sum(), 3 * J)).astype(np.float32)
    out2, mv2, _ = _raw(dev, other, runs, fc, beta, 0.1)
    assert out2[:F][keep].tobytes() == out[:F][keep].tobytes() and mv2[:F][keep].tobytes() == mv[:F][keep].tobytes()
    for cut in (79, 85, 86, 87, 100, 137):                                  # (85, 86, 87: around the ring's first refill)
        later = src.copy()
        later[cut:138] = rng.normal(0.0, 0.7, (138 - cut, 3 * J)).astype(np.float32)
        out3, mv3, _ = _raw(dev, later, runs, fc, beta, 0.1)
        assert out3[78:cut].tobytes() == out[78:cut].tobytes() and mv3[78:cut].tobytes() == mv[78:cut].tobytes(), cut
        assert out3[cut].tobytes() != out[cut].tobytes(), cut


def slow_rows(rng, rows, J, bones, L):
    """Rigid rows [rows, 3 J] (float32) of a skeleton whose roots start within 2 m and drift, and whose bones turn slowly."""
    children = [c for c, _ in bones]
    roots = {j: rng.uniform(-2.0, 2.0, 3) for j in range(J) if j not in children}
    dirs = rng.normal(size=(len(bones), 3))
    out = np.zeros((rows, J, 3))
    for f in range(rows):
        for j in roots:
            roots[j] = roots[j] + rng.normal(0.0, 0.02, 3)
            out[f, j] = roots[j]
        dirs = dirs + rng.normal(0.0, 0.05, dirs.shape)
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        for (c, p), d, l in zip(bones, dirs, L):
            out[f, c] = out[f, p] + float(l) * d
    return out.reshape(rows, 3 * J).astype(np.float32)


@pytest.mark.parametrize("tree", ["upper", "lower"])
def test_one_euro_bones_against_the_restatement(dev, tree):
    from mmego_amd import ops
    J, bones = _trees()[tree]
    rng = np.random.default_rng(J)
    L = rng.uniform(0.05, 0.55, len(bones)).astype(np.float32)
    src = slow_rows(rng, F, J, bones.tolist(), L)
    runs = ops.one_euro_runs(SEG)
    copied = np.repeat(runs[1] == 0, np.diff(runs[0]))
    firsts = runs[0][:-1]
    filtered = ~copied
    filtered[firsts] = False
    roots = [j for j in range(J) if j not in bones[:, 0]]
    worst = worst_m = worst_len = 0.0
    for case, (fc, beta) in enumerate(PARAMS):
        pad_s, pad_d = (0, 0) if case % 2 else (3, 5)
        want, want_m, want_fb = oref.one_euro_bones(src, runs, fc, beta, 0.1, bones.tolist(), L)
        assert (want_fb == 0).all()
        out, mv, fb = _raw(dev, src, runs, fc, beta, 0.1, pad_s, pad_d, bones=bones, L=L)
        _untouched(out, mv, F, 3 * J, fb)
        worst, worst_m = max(worst, ref.within(out[:F, :3 * J], want)), max(worst_m, ref.within(mv[:F], want_m))
        assert (fb[:F] == 0).all()
        assert out[:F, :3 * J][copied].tobytes() == src[copied].tobytes() and out[:F, :3 * J][firsts].tobytes() == src[firsts].tobytes()
        assert (mv[:F][copied] == 0.0).all() and (mv[:F][firsts] == 0.0).all()
        x = out[:F, :3 * J].astype(np.float64).reshape(F, J, 3)
        length = np.linalg.norm(x[:, bones[:, 0]] - x[:, bones[:, 1]], axis=2)
        worst_len = max(worst_len, np.abs(length[filtered] - L.astype(np.float64)).max())
        # the roots: the column form's bits
        col, _, _ = _raw(dev, src, runs, fc, beta, 0.1, pad_s, pad_d)
        cols = np.asarray([3 * r + t for r in roots for t in range(3)])
        assert out[:F][:, cols].tobytes() == col[:F][:, cols].tobytes()
        # two launches, the same bits; without moved and fallback the same dst, those buffers untouched
        out2, mv2, fb2 = _raw(dev, src, runs, fc, beta, 0.1, pad_s, pad_d, bones=bones, L=L)
        assert out2.tobytes() == out.tobytes() and mv2.tobytes() == mv.tobytes() and fb2.tobytes() == fb.tobytes()
        out3, mv3, fb3 = _raw(dev, src, runs, fc, beta, 0.1, pad_s, pad_d, moved=False, bones=bones, L=L, fallback=False)
        assert out3.tobytes() == out.tobytes() and (mv3 == SENT).all() and (fb3 == -7).all()
    print("one_euro_bones %s: dst worst error / bound %.3f, moved %.3f, worst | |bone| - L | %.3e m" % (tree, worst, worst_m, worst_len))
    assert worst <= 1.0 and worst_m <= 1.0 and worst_len <= RIGID


def test_a_bone_that_reverses_every_frame_at_alpha_one_half_takes_the_fallback(dev):
    """fc = 1 / (2 pi), beta = 0: alpha = 1/2.  The bone's vector alternates +v, -v, so vhat_1 = v + (-2 v) / 2 = 0: the run's second
    frame keeps its own direction -v and counts one fallback; from then on vhat = v / 2, -v / 4, 3 v / 8, ... never vanishes (worked
    out with scripts/one_euro_host_check.hip; the restatement below shows the same counts on its own)."""
    bones, L = np.asarray([[1, 0]], np.int32), np.asarray([0.25], np.float32)
    n = 6
    src = np.zeros((n, 2, 3), np.float32)
    src[:, 0] = [0.5, -0.25, 1.0]
    src[:, 1] = src[:, 0] + np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None] * np.asarray([0.25, 0.0, 0.0], np.float32)
    src = src.reshape(n, 6)
    runs = (np.asarray([0, n], np.int64), np.asarray([1], np.int32))
    fc = 1.0 / (2.0 * np.pi)
    want, want_m, want_fb = oref.one_euro_bones(src, runs, fc, 0.0, 0.1, bones.tolist(), L)
    assert want_fb.tolist() == [0, 1, 0, 0, 0, 0]
    assert np.allclose(want.reshape(n, 2, 3)[:, 1, 0], [0.75, 0.25, 0.75, 0.25, 0.75, 0.25], atol=1e-12)
    out, mv, fb = _raw(dev, src, runs, fc, 0.0, 0.1, bones=bones, L=L)
    assert fb[:n].tolist() == [0, 1, 0, 0, 0, 0]
    assert ref.within(out[:n, :6], want) <= 1.0 and ref.within(mv[:n], want_m) <= 1.0


def test_refusals_come_before_any_launch(dev):
    from mmego_amd import hip, ops, skeleton
    rng = np.random.default_rng(2)
    J, rows = 15, 12
    src = _d(dev, rng.normal(0.0, 0.7, (rows, 3 * J)).astype(np.float32))
    dst = torch.full((rows, 3 * J), SENT, dtype=torch.float32, device=dev)
    mv = torch.full((rows,), SENT, dtype=torch.float32, device=dev)
    fb = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    runs = ops.one_euro_runs(np.zeros(rows, np.int32))
    L = np.full(14, 0.2, np.float32)
    i64, i32 = (lambda *v: np.asarray(v, np.int64)), (lambda *v: np.asarray(v, np.int32))
    buf = torch.zeros((2 * rows, 3 * J), dtype=torch.float32, device=dev)
    bad = [("dst overlapping src", lambda: ops.one_euro(buf[:rows], runs, 1.0, 0.0, 0.1, buf[rows - 1:2 * rows - 1])),
           ("dst is src", lambda: ops.one_euro(src, runs, 1.0, 0.0, 0.1, src)),
           ("runs that stop short", lambda: ops.one_euro(src, (i64(0, rows - 1), i32(1)), 1.0, 0.0, 0.1, dst)),
           ("runs that do not start at 0", lambda: ops.one_euro(src, (i64(1, rows), i32(1)), 1.0, 0.0, 0.1, dst)),
           ("an empty run", lambda: ops.one_euro(src, (i64(0, 4, 4, rows), i32(1, 1, 1)), 1.0, 0.0, 0.1, dst)),
           ("descending runs", lambda: ops.one_euro(src, (i64(0, 8, 4, rows), i32(1, 1, 1)), 1.0, 0.0, 0.1, dst)),
           ("int32 offsets", lambda: ops.one_euro(src, (i32(0, rows), i32(1)), 1.0, 0.0, 0.1, dst)),
           ("one flag too many", lambda: ops.one_euro(src, (i64(0, rows), i32(1, 1)), 1.0, 0.0, 0.1, dst)),
           ("fc 0", lambda: ops.one_euro(src, runs, 0.0, 0.0, 0.1, dst)),
           ("fc NaN", lambda: ops.one_euro(src, runs, float("nan"), 0.0, 0.1, dst)),
           ("beta < 0", lambda: ops.one_euro(src, runs, 1.0, -1.0, 0.1, dst)),
           ("beta inf", lambda: ops.one_euro(src, runs, 1.0, float("inf"), 0.1, dst)),
           ("dc 0", lambda: ops.one_euro(src, runs, 1.0, 0.0, 0.0, dst)),
           ("dc NaN", lambda: ops.one_euro(src, runs, 1.0, 0.0, float("nan"), dst)),
           ("a short dst", lambda: ops.one_euro(src, runs, 1.0, 0.0, 0.1, dst[:rows - 1])),
           ("a narrow dst", lambda: ops.one_euro(src, runs, 1.0, 0.0, 0.1, dst[:, :44])),
           ("rows that are no 3-vectors", lambda: ops.one_euro(src[:, :44], runs, 1.0, 0.0, 0.1, dst)),
           ("a double source", lambda: ops.one_euro(src.double(), runs, 1.0, 0.0, 0.1, dst)),
           ("a host source", lambda: ops.one_euro(src.cpu(), runs, 1.0, 0.0, 0.1, dst)),
           ("an int moved", lambda: ops.one_euro(src, runs, 1.0, 0.0, 0.1, dst, fb)),
           ("a short moved", lambda: ops.one_euro(src, runs, 1.0, 0.0, 0.1, dst, mv[:rows - 1])),
           ("a bone before its parent", lambda: ops.one_euro_bones(src, runs, 1.0, 0.0, 0.1, skeleton.WALK_UPPER[::-1], L, dst)),
           ("a bone length of 0", lambda: ops.one_euro_bones(src, runs, 1.0, 0.0, 0.1, skeleton.WALK_UPPER, L * 0, dst)),
           ("a float fallback", lambda: ops.one_euro_bones(src, runs, 1.0, 0.0, 0.1, skeleton.WALK_UPPER, L, dst, mv, mv)),
           ("bones form, bad runs", lambda: ops.one_euro_bones(src, (i64(0, rows - 1), i32(1)), 1.0, 0.0, 0.1, skeleton.WALK_UPPER, L, dst)),
           ("bones form, fc 0", lambda: ops.one_euro_bones(src, runs, 0.0, 0.0, 0.1, skeleton.WALK_UPPER, L, dst))]
    for name, call in bad:
        with pytest.raises((ValueError, IndexError)):
            call()
            pytest.fail(name)
    # the entry points themselves: the library's error code, nothing launched
    off, on = _d(dev, runs[0]), _d(dev, runs[1])
    bd, ld = _d(dev, np.asarray(skeleton.WALK_UPPER, np.int32)), _d(dev, L)
    good = dict(src=src, lds=45, F=rows, J=J, run_off=off, run_on=on, R=1, fc=1.0, beta=0.0, dc=0.1, dst=dst, ldd=45, moved=mv)
    tail = dict(bones=bd, bone_len=ld, NB=14)
    for change in (dict(src=None), dict(run_off=None), dict(run_on=None), dict(dst=None), dict(F=0), dict(J=0), dict(J=22), dict(lds=44),
                   dict(ldd=44), dict(R=0), dict(R=rows + 1), dict(fc=0.0), dict(fc=float("nan")), dict(fc=float("inf")), dict(beta=-1.0),
                   dict(beta=float("nan")), dict(dc=0.0), dict(dc=float("inf")), dict(dst=src)):
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("one_euro", *[a[k] for k in good])
        b = dict(a, fallback=fb)
        order = [k for k in good if k not in ("dst", "ldd", "moved")] + ["bones", "bone_len", "NB", "dst", "ldd", "moved", "fallback"]
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("one_euro_bones", *[dict(b, **tail)[k] for k in order])
    for change in (dict(NB=-1), dict(NB=15), dict(bones=None), dict(bone_len=None)):
        b = dict(good, fallback=fb, **dict(tail, **change))
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("one_euro_bones", *[b[k] for k in order])
    torch.cuda.synchronize()
    assert (dst == SENT).all() and (mv == SENT).all() and (fb == -7).all(), "a refused call leaves every output untouched"
