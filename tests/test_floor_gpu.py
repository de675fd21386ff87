"""GPU: the floor kernels (ops.floor_stats / ops.floor_clamp) against the float64 restatement of tests/floor_ref.py, their refusals, and
dense inference with floor=(mode, contact_cm, margin_cm) and `main.py --infer --dense --floor clamp` on the synthetic Sample_data tree of
tests/test_dense_infer_gpu.py (recordings of 23, 20, 7 and 41 frames, frame_no = 20, nets from torch.manual_seed, the recorded head pose).

Bounds.  Statistics: 4e-6 m on the float columns (four roundings of magnitudes <= 8 at 2^-24, for |x_i|, |d| <= 4); flags exact except
where the reference height lies within 1e-5 of 0 or of H without being it.  Clamp: 2e-5 m against the reference (the project's joint
bound) where the knee stands 5 cm or more off the hip-ankle line -- moving the ankle shifts the knee by at most l1 / b <= 10 times as
much, and 1e-6 m of rounding in the ankle then stays under 1e-5 --, bone lengths to 2e-6 m, the foot bone's vector to 2e-7, heights
from the stored floats >= margin - 4e-6, the lift within 4e-6.  Pass: rates exact, lengths to 1e-3 cm (the project's bar for a figure)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import floor_ref as fref
from conftest import ROOT
from test_dense_infer_gpu import LENGTHS, F, T, _World, _make_dataset
from test_dense_smooth_gpu import _same

pytestmark = pytest.mark.gpu

H = 0.0625
DEV = "cuda:0"


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


@pytest.fixture(scope="module")
def stat_case():
    """37 random rows in segments of 1, 2 and 34 rows with two rows of the last one outside every segment, and two built rows whose
    heights are exactly 0 and exactly H.  -> the float32 inputs and the reference on them."""
    rng = np.random.default_rng(11)
    lo, ground = fref.random_legs(rng, 37)
    lo = (lo + rng.normal(0.0, 0.05, lo.shape)).astype(np.float32)
    tgt = rng.normal(0.0, 0.5, (37, 21, 3)) + np.array([0.0, 0.0, 0.8])
    tgt[:, [15, 19]] = lo.reshape(37, 8, 3)[:, [3, 7]] + rng.normal(0.0, 0.03, (37, 2, 3))
    tgt = tgt.reshape(37, 63).astype(np.float32)
    ground = ground.astype(np.float32)
    contact = rng.integers(0, 2, (37, 2)).astype(np.float32)
    seg = np.concatenate([[0], [1, 1], np.full(34, 2)]).astype(np.int32)
    seg[[17, 18]] = -1
    # built: n = (0, 0, 1), d = 0; row 37 the predicted feet at z = 0 and z = H, the target's at H and 0; row 38 the other way round
    built_lo, built_tgt = np.zeros((2, 8, 3), np.float32), np.zeros((2, 21, 3), np.float32)
    built_lo[:, :, :2], built_tgt[:, :, :2] = 0.3, -0.2
    built_lo[0, 3, 2], built_lo[0, 7, 2], built_tgt[0, 15, 2], built_tgt[0, 19, 2] = 0.0, H, H, 0.0
    built_lo[1, 3, 2], built_lo[1, 7, 2], built_tgt[1, 15, 2], built_tgt[1, 19, 2] = H, 0.0, 0.0, H
    lo = np.concatenate([lo, built_lo.reshape(2, 24)])
    tgt = np.concatenate([tgt, built_tgt.reshape(2, 63)])
    ground = np.concatenate([ground, np.array([[0, 0, 1, 0], [0, 0, 1, 0]], np.float32)])
    contact = np.concatenate([contact, np.array([[1, 1], [1, 0]], np.float32)])
    seg = np.concatenate([seg, [3, 3]]).astype(np.int32)
    assert np.abs(lo).max() <= 4 and np.abs(tgt).max() <= 4 and np.abs(ground).max() <= 4
    ref, hp, ht = fref.stats(lo, tgt, ground, contact, seg, H)
    return dict(lo=lo, tgt=tgt, ground=ground, contact=contact, seg=seg, ref=ref, hp=hp, ht=ht)


FLOAT_COLS, FLAG_COLS = (0, 1, 6, 7), (2, 3, 4, 5, 8, 9, 10)


def test_stats_against_the_restatement(stat_case):
    from mmego_amd import ops
    c = stat_case
    rows = len(c["lo"])
    out = torch.full((rows, ops.FLOOR_W), 7.0, device=DEV)
    ops.floor_stats(_dev(c["lo"]), _dev(c["tgt"]), _dev(c["ground"]), _dev(c["contact"]), c["seg"], H, out)
    got, ref = out.cpu().numpy().astype(np.float64).reshape(rows, 2, 11), c["ref"].reshape(rows, 2, 11)
    # the pairs (row, foot) whose flags may legitimately differ: a reference height within 1e-5 of a threshold without sitting on it
    h = np.stack([c["hp"], c["ht"]], axis=2)
    close = ((np.abs(h) < 1e-5) & (h != 0.0)) | ((np.abs(h - H) < 1e-5) & (h != H))
    doubt = close.any(axis=2)
    assert doubt.sum() <= 0.01 * doubt.size, "the cap on the pairs left out, on the reference alone"
    worst = np.abs(got[:, :, FLOAT_COLS] - ref[:, :, FLOAT_COLS]).max()
    print("float columns differ from the reference by at most %.3e m; %d of %d pairs left out of the flags" % (worst, doubt.sum(), doubt.size))
    assert worst <= 4e-6
    assert np.array_equal(got[:, :, FLAG_COLS][~doubt], ref[:, :, FLAG_COLS][~doubt])
    # rows outside a segment: all zeros; the built rows pin the strict comparisons
    assert not got[c["seg"] < 0].any() and got[c["seg"] >= 0].any(axis=(1, 2)).all()
    a, b = got[37], got[38]
    assert a[0, 2] == 0 and a[0, 3] == 1 and a[0, 4] == 1 and a[0, 8] == 0 and a[0, 9] == 0 and a[0, 10] == 0, "hp = 0, ht = H"
    assert a[1, 2] == 0 and a[1, 3] == 0 and a[1, 4] == 0 and a[1, 8] == 0 and a[1, 9] == 1 and a[1, 10] == 1, "hp = H, ht = 0"
    assert b[0, 3] == 0 and b[1, 3] == 1 and b[1, 4] == 0 and b[1, 5] == 0 and b[1, 9] == 0
    assert a[0, 0] == np.float32(H) and a[0, 1] == 0 and a[0, 6] == 0 and a[1, 6] == np.float32(H)


def test_stats_of_strided_rows_and_a_device_seg(stat_case):
    from mmego_amd import ops
    c = stat_case
    rows = len(c["lo"])
    args = (_dev(c["ground"]), _dev(c["contact"]))
    packed = ops.floor_stats(_dev(c["lo"]), _dev(c["tgt"]), *args, c["seg"], H, torch.empty((rows, ops.FLOOR_W), device=DEV))
    wide_lo, wide_tgt = torch.full((rows, 32), 9.0, device=DEV), torch.full((rows, 70), 9.0, device=DEV)
    wide_lo[:, :24], wide_tgt[:, :63] = _dev(c["lo"]), _dev(c["tgt"])
    strided = ops.floor_stats(wide_lo[:, :24], wide_tgt[:, :63], *args, _dev(c["seg"], torch.int32), H,
                              torch.empty((rows, ops.FLOOR_W), device=DEV))
    assert torch.equal(packed, strided)


@pytest.fixture(scope="module")
def clamp_case():
    """64 rows of random legs in float32, row 10 outside every segment, row 20 without a normal; the reference at both margins."""
    rows, ground = fref.random_legs(np.random.default_rng(5), 64)
    rows, ground = rows.astype(np.float32), ground.astype(np.float32)
    ground[20, :3] = 0.0
    seg = np.zeros(64, dtype=np.int32)
    seg[10] = -1
    return dict(rows=rows, ground=ground, seg=seg, ref={m: fref.clamp(rows, ground, seg, m) for m in (0.0, 0.02)})


@pytest.mark.parametrize("margin", [0.0, 0.02])
def test_clamp_against_the_restatement(clamp_case, margin):
    from mmego_amd import ops
    c = clamp_case
    ref, ref_lift, ref_fb, legs = c["ref"][margin]
    src = _dev(c["rows"])
    dst, lifted, fb = torch.full((64, 24), 5.0, device=DEV), torch.full((64,), 5.0, device=DEV), torch.full((64,), 5, dtype=torch.int32, device=DEV)
    ops.floor_clamp(src, _dev(c["ground"]), c["seg"], margin, dst, lifted, fb)
    got, lifted, fb = dst.cpu().numpy(), lifted.cpu().numpy(), fb.cpu().numpy()
    x, y, r64 = c["rows"].reshape(64, 8, 3), got.reshape(64, 8, 3), ref.reshape(64, 8, 3)
    # on the reference alone: the rows that are compared joint by joint
    raised = np.array([both[0] is not None and any(res["lift"] > 0 for res in both) for both in legs])
    sound = np.array([both[0] is not None and all(res["lift"] == 0 or (res["fallback"] == 0 and res["b"] >= 0.05) for res in both)
                      for both in legs])
    assert raised.sum() >= 16 and (raised & sound).sum() >= 0.9 * raised.sum()
    worst = np.abs(got[raised & sound].astype(np.float64) - ref[raised & sound]).max()
    print("margin %g: %d rows raised, %d compared; joints differ from the reference by at most %.3e m" % (margin, raised.sum(),
                                                                                                          (raised & sound).sum(), worst))
    assert worst <= 2e-5
    # rows outside a segment, rows without a plane: bit for bit
    for r in (10, 20):
        assert got[r].tobytes() == c["rows"][r].tobytes() and lifted[r] == 0.0
    assert fb[10] == 0 and fb[20] == 2
    worst_len = worst_foot = 0.0
    lowest = np.inf
    for r in range(64):
        if legs[r][0] is None:
            continue
        pl = fref.plane(c["ground"][r])
        for (h, k, a, t), res in zip(fref.LEGS, legs[r]):
            assert y[r, h].tobytes() == x[r, h].tobytes(), "the hips are copies"
            if res["lift"] == 0.0:
                assert y[r, [k, a, t]].tobytes() == x[r, [k, a, t]].tobytes(), "a leg above the margin is a copy"
                continue
            if res["fallback"]:
                continue
            d = lambda p, q, z: np.linalg.norm(z[r, p].astype(np.float64) - z[r, q])
            worst_len = max(worst_len, abs(d(k, h, y) - d(k, h, x)), abs(d(a, k, y) - d(a, k, x)))
            worst_foot = max(worst_foot, np.abs((y[r, t].astype(np.float64) - y[r, a]) - (x[r, t].astype(np.float64) - x[r, a])).max())
            lowest = min(lowest, fref.height(pl, y[r, a].astype(np.float64)) - margin, fref.height(pl, y[r, t].astype(np.float64)) - margin)
    print("margin %g: bone lengths kept to %.3e m, the foot bone to %.3e, lowest height above the margin %.3e; lift differs by %.3e" % (
        margin, worst_len, worst_foot, lowest, np.abs(lifted - ref_lift).max()))
    assert worst_len <= 2e-6 and worst_foot <= 2e-7 and lowest >= -4e-6
    assert np.abs(lifted - ref_lift).max() <= 4e-6
    edge = np.array([min([np.inf] + [res["edge"] for res in both if res is not None]) for both in legs])
    assert np.array_equal(fb[edge > 1e-5], ref_fb[edge > 1e-5])
    # in place: the bits of the out-of-place call; the columns behind the row stay
    wide = torch.full((64, 30), 3.0, device=DEV)
    wide[:, :24] = src
    lifted2 = torch.empty(64, device=DEV)
    ops.floor_clamp(wide[:, :24], _dev(c["ground"]), c["seg"], margin, wide[:, :24], lifted2)
    assert torch.equal(wide[:, :24], dst) and (wide[:, 24:] == 3.0).all() and np.array_equal(lifted2.cpu().numpy(), lifted)


def _one_leg(Hp, K, A, T, ground=(0.0, 0.0, 1.0, 0.0), margin=0.0):
    from mmego_amd import ops
    row = np.zeros((1, 8, 3), np.float32)
    row[0, :4] = [Hp, K, A, T]
    row[0, 4:] = np.array([[0.0, 0.2, 0.9], [0.05, 0.2, 0.5], [0.0, 0.2, 0.1], [0.1, 0.2, 0.05]])      # the other leg stands above the floor
    src = _dev(row.reshape(1, 24))
    dst, lifted, fb = torch.empty((1, 24), device=DEV), torch.empty(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.floor_clamp(src, _dev(np.array([ground], np.float32)), np.zeros(1, np.int32), margin, dst, lifted, fb)
    out = dst.cpu().numpy().reshape(8, 3)
    assert out[4:].tobytes() == row[0, 4:].tobytes() and out[0].tobytes() == row[0, 0].tobytes()
    same = src.clone()
    ops.floor_clamp(same, _dev(np.array([ground], np.float32)), np.zeros(1, np.int32), margin, same)
    assert torch.equal(same, dst), "dst is src: the bits of the out-of-place call"
    return out.astype(np.float64), float(lifted[0]), int(fb[0]), row[0].astype(np.float64)


def test_built_legs():
    # the hip under the floor, the target out of reach: the ankle at reach along u, one fallback, finite
    out, lift, fb, x = _one_leg([0.0, 0.0, -1.0], [0.0, 0.1, -1.4], [0.0, 0.0, -1.8], [0.1, 0.0, -1.85])
    l1, l2 = np.linalg.norm(x[1] - x[0]), np.linalg.norm(x[2] - x[1])
    assert fb == 1 and np.isfinite(out).all() and abs(lift - 1.85) <= 4e-6
    u = (x[2] + 1.85 * np.array([0, 0, 1.0]) - x[0])
    u /= np.linalg.norm(u)
    assert np.abs(out[2] - (x[0] + (l1 + l2) * (1 - 1e-6) * u)).max() <= 2e-6
    assert np.abs((out[3] - out[2]) - (x[3] - x[2])).max() <= 2e-7
    # a straight vertical leg pushed up: the knee goes where the foot points, the lengths stay
    out, lift, fb, x = _one_leg([0.0, 0.0, 0.9], [0.0, 0.0, 0.5], [0.0, 0.0, 0.1], [0.1, 0.0, -0.05])
    assert fb == 0 and abs(lift - 0.05) <= 4e-6 and out[1, 0] > 0.05 and abs(out[1, 1]) <= 1e-6
    assert abs(np.linalg.norm(out[1] - out[0]) - 0.4) <= 2e-6 and abs(np.linalg.norm(out[2] - out[1]) - 0.4) <= 2e-6
    assert out[2, 2] >= 0.15 - 4e-6 and out[3, 2] >= 0.0
    # the same with a vertical foot bone: the axis rule (x, the first of the two axes u does not lean on), finite
    out, lift, fb, x = _one_leg([0.0, 0.0, 0.9], [0.0, 0.0, 0.5], [0.0, 0.0, 0.1], [0.0, 0.0, -0.05])
    assert fb == 0 and np.isfinite(out).all() and out[1, 0] > 0.05 and abs(out[1, 1]) <= 1e-6
    assert abs(np.linalg.norm(out[1] - out[0]) - 0.4) <= 2e-6 and abs(np.linalg.norm(out[2] - out[1]) - 0.4) <= 2e-6


def test_every_refusal_comes_before_any_launch(monkeypatch, stat_case):
    from mmego_amd import hip, ops
    c = stat_case
    rows = len(c["lo"])
    lo, tgt, ground, contact = _dev(c["lo"]), _dev(c["tgt"]), _dev(c["ground"]), _dev(c["contact"])
    out, seg = torch.empty((rows, ops.FLOOR_W), device=DEV), c["seg"]
    dst, lifted, fb = torch.empty((rows, 24), device=DEV), torch.empty(rows, device=DEV), torch.zeros(rows, dtype=torch.int32, device=DEV)
    wide = torch.zeros((rows + 1, 48), device=DEV)

    def no_launch(name, *args):
        raise AssertionError("mmego_%s was launched" % name)

    monkeypatch.setattr(hip, "_launch", no_launch)
    bad_stats = [
        dict(lo=lo[:, :23]), dict(lo=lo.double()), dict(lo=lo.cpu()), dict(lo=lo.t().contiguous().t()), dict(lo=lo[0]),
        dict(tgt=tgt[:, :60]), dict(tgt=tgt[:-1]), dict(tgt=tgt.cpu()),
        dict(ground=ground[:, :3]), dict(ground=ground[:-1]), dict(ground=wide[:rows, :4]), dict(ground=ground.cpu()),
        dict(contact=contact[:, :1]), dict(contact=contact.to(torch.uint8)), dict(contact=wide[:rows, :2]),
        dict(seg=seg[:-1]), dict(seg=seg.astype(np.int64)), dict(seg=torch.as_tensor(seg)), dict(seg=_dev(seg, torch.int64)), dict(seg=list(seg)),
        dict(H=0.0), dict(H=-0.01), dict(H=float("nan")), dict(H=float("inf")), dict(H="0.06"), dict(H=True),
        dict(out=out[:, :21]), dict(out=out[:-1]), dict(out=wide[:rows, :22]), dict(out=out.cpu()),
    ]
    good = dict(lo=lo, tgt=tgt, ground=ground, contact=contact, seg=seg, H=H, out=out)
    for bad in bad_stats:
        with pytest.raises(ValueError, match="floor_stats"):
            ops.floor_stats(**dict(good, **bad))
    flat = wide.view(-1)
    bad_clamp = [
        dict(src=lo[:, :23]), dict(src=lo.double()), dict(src=lo.cpu()), dict(src=lo[0]),
        dict(ground=ground[:, :3]), dict(ground=ground[:-1]), dict(ground=ground.cpu()),
        dict(seg=seg[:-1]), dict(seg=seg.astype(np.int64)), dict(seg=torch.as_tensor(seg)),
        dict(margin=-0.01), dict(margin=float("nan")), dict(margin=float("inf")), dict(margin="0"), dict(margin=False),
        dict(dst=dst[:, :23]), dict(dst=dst[:-1]), dict(dst=dst.cpu()),
        dict(src=wide[:rows, :24], dst=wide[:rows, 12:36]), dict(src=wide[:rows, :24], dst=wide[1:, :24]),
        dict(src=flat[:rows * 24].view(rows, 24), dst=wide[:rows, :24]),
        dict(lifted=lifted[:-1]), dict(lifted=lifted.double()), dict(lifted=lifted.cpu()), dict(lifted=wide[:rows, 0]),
        dict(fallback=fb[:-1]), dict(fallback=lifted), dict(fallback=fb.cpu()),
    ]
    good = dict(src=lo, ground=ground, seg=seg, margin=0.0, dst=dst, lifted=lifted, fallback=fb)
    for bad in bad_clamp:
        with pytest.raises(ValueError, match="floor_clamp"):
            ops.floor_clamp(**dict(good, **bad))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The tree, its PosePC with the per-frame clouds, seeded nets; after a first pass the floor of every frame is set to z = the median
    predicted foot height (about half the feet then lie under it) and the flags are drawn at random.  The passes are computed once."""
    assert torch.cuda.is_available()
    from mmego_amd import dense, nets, processors
    from mmego_amd.config import ConfigDemo
    from mmego_amd.data import PosePC
    w = _World()
    w.tmp = tmp_path_factory.mktemp("dense_floor")
    w.data = str(w.tmp / "Sample_data")
    _make_dataset(w.data, np.random.default_rng(0))
    np.random.seed(3)
    w.ds = PosePC(train=False, vis=True, keep_frames=True, batch_length=T, root=w.data)
    assert len(w.ds.frame_npts_) == F and w.ds.frame_ground_.shape == (F, 4) and w.ds.frame_contact_.shape == (F, 2)
    assert np.array_equal(w.ds.frame_ground_, np.tile(np.float32([0, 0, -1, 1]), (F, 1))) and np.array_equal(w.ds.frame_contact_, np.tile(np.uint8([1, 0]), (F, 1)))
    keep = ConfigDemo.gt_head_pose
    ConfigDemo.gt_head_pose = True
    try:
        w.base = processors._Base(ConfigDemo, make_dirs=False)
    finally:
        ConfigDemo.gt_head_pose = keep
    w.dev = w.base.device
    torch.manual_seed(0)
    w.up, w.lo = nets.UpperNet().to(w.dev).eval(), nets.LowerNet(64).to(w.dev).eval()
    torch.save(w.up.state_dict(), w.tmp / "upper.pth")
    torch.save(w.lo.state_dict(), w.tmp / "lower.pth")
    w.runs = {}

    def run(space=None, metrics="reference", **more):
        key = (space, metrics, tuple(sorted(more.items())))
        if key not in w.runs:
            if space is not None:
                more = dict(more, blend_space=space)
            w.runs[key] = dense.dense_infer(w.base, None, w.up, w.lo, w.ds, 3, batch_size=4, metrics=metrics, **more)
        return w.runs[key]

    w.run = run
    _, a = run()
    cov = a["covered"] > 0
    w.level = float(np.median(a["lower"][cov][:, [3, 7], 2]))
    w.ds.frame_ground_ = np.tile(np.float32([0.0, 0.0, 1.0, -w.level]), (F, 1))
    w.ds.frame_contact_ = np.random.default_rng(4).integers(0, 2, (F, 2)).astype(np.uint8)
    w.runs.clear()
    return w


def _figures(feet, target_feet, ground, contact, Hc):
    """The floor figures in float64 from feet [n, 2, 3], the target's feet, planes [n, 4], flags [n, 2]: per foot and pooled."""
    g = ground.astype(np.float64)
    hp = np.einsum("fki,fi->fk", feet.astype(np.float64), g[:, :3]) + g[:, 3:4]
    ht = np.einsum("fki,fi->fk", target_feet.astype(np.float64), g[:, :3]) + g[:, 3:4]
    c = contact.astype(np.float64)
    ratio = lambda a, b, s=1.0: None if b == 0 else float(a) / float(b) * s
    res = {}
    for name, sl in (("", slice(None)), ("0", slice(0, 1)), ("1", slice(1, 2))):
        p, t, f = hp[:, sl], ht[:, sl], c[:, sl]
        res[name] = dict(foot_height_err_cm=ratio(np.abs(p - t).sum(), p.size, 100), penetration_rate=ratio((p < 0).sum(), p.size),
                         penetration_cm=ratio(-p[p < 0].sum(), (p < 0).sum(), 100), contact_precision=ratio(((p < Hc) * f).sum(), (p < Hc).sum()),
                         contact_recall=ratio(((p < Hc) * f).sum(), f.sum()), hover_cm=ratio((f * np.maximum(p, 0)).sum(), f.sum(), 100),
                         target_penetration_rate=ratio((t < 0).sum(), t.size), target_penetration_cm=ratio(-t[t < 0].sum(), (t < 0).sum(), 100),
                         target_contact_precision=ratio(((t < Hc) * f).sum(), (t < Hc).sum()), target_contact_recall=ratio(((t < Hc) * f).sum(), f.sum()))
    return res, hp


RATES = ("penetration_rate", "contact_precision", "contact_recall", "target_penetration_rate", "target_contact_precision", "target_contact_recall")


def _hold(summary, want, prefix="", keys=None):
    for k, v in want[""].items():
        if keys is not None and k not in keys:
            continue
        name = k if k.startswith("target_") else prefix + k
        for got, ref in ((summary[name], v), (summary[name + "_per_foot"][0], want["0"][k]), (summary[name + "_per_foot"][1], want["1"][k])):
            if ref is None or k in RATES:
                assert got == ref, (name, got, ref)
            else:
                assert abs(got - ref) <= 1e-3, (name, got, ref)


def test_floor_none_is_the_call_without_the_argument(world):
    s0, a0 = world.run(None, "full")
    s1, a1 = world.run(None, "full", floor=None)
    _same(s0, s1)
    _same(a0, a1)
    assert not any("floor" in k or "penetration" in k or "clamp" in k or k in ("ground", "foot_height", "foot_contact", "lifted")
                   for k in list(s1) + list(a1))
    assert a1["plan"]._floor is None, "nothing was uploaded"


@pytest.mark.parametrize("space", [None, "rot"])
def test_measure_against_float64(world, space):
    from mmego_amd import dense
    s0, a0 = world.run(space)
    s, a = world.run(space, floor=("measure", 6, 0))
    cov = a["covered"] > 0
    assert s["floor"] == ("measure", 6.0, 0.0) and a["pred"].tobytes() == a0["pred"].tobytes()
    for k, v in s0.items():
        assert np.array_equal(v, s[k]) if isinstance(v, np.ndarray) else v == s[k], k
    assert set(a) - set(a0) == {"foot_height", "ground", "foot_contact"}
    assert np.array_equal(a["ground"], world.ds.frame_ground_) and np.array_equal(a["foot_contact"], world.ds.frame_contact_.astype(np.float32))
    assert np.array_equal(a["pred"][cov][:, [15, 19]], a["lower"][cov][:, [3, 7]])
    want, hp = _figures(a["pred"][cov][:, [15, 19]], a["target"][cov][:, [15, 19]], a["ground"][cov], a["foot_contact"][cov], 0.06)
    print("penetration rate %.3f depth %.3f cm; precision %s recall %s; target rate %.3f" % (
        s["penetration_rate"], s["penetration_cm"], s["contact_precision"], s["contact_recall"], s["target_penetration_rate"]))
    assert 0.3 <= s["penetration_rate"] <= 0.7, "the plane stands at the median foot height"
    _hold(s, want)
    assert a["foot_height"].shape == (F, 2) and a["foot_height"].dtype == np.float32
    assert np.array_equal(a["foot_height"][cov], hp.astype(np.float32)) and np.isnan(a["foot_height"][~cov]).all()
    # the window rows, with the planes and flags of their frames
    plan = a["plan"]
    win = a["win_lo"].cpu().numpy().reshape(-1, 8, 3)
    rf = plan.row_frame
    want_w, _ = _figures(win[:, [3, 7]], a["target"][rf][:, [15, 19]], a["ground"][rf], a["foot_contact"][rf], 0.06)
    _hold(s, want_w, "single_", dense.FLOOR_KEYS)
    assert set(s) - set(s0) == ({p + k + t for p in ("", "single_") for k in dense.FLOOR_KEYS for t in ("", "_per_foot")}
                                | {k + t for k in dense.FLOOR_TARGET_KEYS for t in ("", "_per_foot")} | {"floor"})


@pytest.mark.parametrize("smooth", [None, (2, 2, "gauss")])
def test_clamp_keeps_the_saved_feet_off_the_floor(world, smooth):
    more = {} if smooth is None else dict(smooth=smooth)
    sm, am = world.run(None, "full", floor=("measure", 6, 0), **more)
    s, a = world.run(None, "full", floor=("clamp", 6, 0), **more)
    cov = a["covered"] > 0
    assert s["floor"] == ("clamp", 6.0, 0.0)
    assert set(a) - set(am) == {"pred_unclamped", "lifted", "floor_fallback"}
    # before the clamp: the measure pass, frames and figures
    assert a["pred_unclamped"].tobytes() == am["pred"].tobytes()
    for k in ("all_cm", "upper_cm", "lower_cm", "accel_cm", "penetration_rate", "penetration_cm", "foot_height_err_cm", "hover_cm"):
        assert s["unclamped_" + k] == sm[k], k
    assert s["unclamped_per_joint_cm"].tobytes() == sm["per_joint_cm"].tobytes() and s["unclamped_penetration_rate_per_foot"] == sm["penetration_rate_per_foot"]
    for k in ("target_penetration_rate", "target_contact_recall", "single_penetration_rate", "single_all_cm", "upper_cm"):
        assert s[k] == sm[k], k
    # the saved frames: nothing under the floor where no leg fell back; uncovered frames NaN; the joints outside the legs untouched
    ok = cov & (a["floor_fallback"] == 0)
    assert ok.any() and s["floor_fallback"] == int(a["floor_fallback"].sum())
    hz = a["pred"][:, [14, 15, 18, 19], 2].astype(np.float64) - np.float64(np.float32(world.level))
    assert (hz[ok] >= 0.0).all(), "ankles and feet of the saved frames respect the floor"
    assert (a["foot_height"][ok] >= 0.0).all() and np.isnan(a["foot_height"][~cov]).all()
    if not (cov & ~ok).any():
        assert s["penetration_rate"] == 0.0 and s["penetration_cm"] is None and s["penetration_rate_per_foot"] == (0.0, 0.0)
    assert np.isnan(a["pred"][~cov]).all() and np.isnan(a["pred_unclamped"][~cov]).all() and not a["lifted"][~cov].any()
    others = [j for j in range(21) if j not in (13, 14, 15, 17, 18, 19)]
    assert a["pred"][cov][:, others].tobytes() == am["pred"][cov][:, others].tobytes(), "the upper joints and the hips"
    up = a["lifted"] > 0
    assert np.array_equal(a["pred"][cov & ~up], am["pred"][cov & ~up]) and (np.abs(a["pred"][up] - am["pred"][up]).max(axis=(1, 2)) > 0).all()
    assert s["lifted_frames"] == int(up.sum()) and 0.3 * cov.sum() <= up.sum() and abs(s["lift_cm"] - a["lifted"][up].astype(np.float64).mean() * 100) <= 1e-3
    # the figures are the clamped frames'
    allj = np.linalg.norm(a["pred"][cov].astype(np.float64) - a["target"][cov], axis=2).mean() * 100
    assert abs(s["all_cm"] - allj) <= 1e-3 and s["all_cm"] != sm["all_cm"]
    want, _ = _figures(a["pred"][cov][:, [15, 19]], a["target"][cov][:, [15, 19]], a["ground"][cov], a["foot_contact"][cov], 0.06)
    _hold(s, want)
    print("smooth %s: %d of %d frames lifted by %.3f cm on average, %d legs out of reach; all_cm %.4f unclamped, %.4f clamped" % (
        smooth, s["lifted_frames"], s["covered_frames"], s["lift_cm"], s["floor_fallback"], s["unclamped_all_cm"], s["all_cm"]))


def test_clamp_under_bones_keeps_the_bone_lengths(world):
    sm, am = world.run("bones", floor=("measure", 6, 0))
    s, a = world.run("bones", floor=("clamp", 6, 0))
    print("bone_dev_cm %.3e unclamped, %.3e clamped; %d frames lifted" % (sm["bone_dev_cm"], s["bone_dev_cm"], s["lifted_frames"]))
    assert s["lifted_frames"] > 0 and abs(s["bone_dev_cm"] - sm["bone_dev_cm"]) <= 1e-3


def test_clamp_under_rot_is_refused(world):
    from mmego_amd import dense
    with pytest.raises(ValueError, match="floor"):
        dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 3, blend_space="rot", floor=("clamp", 6, 0))
    with pytest.raises(ValueError, match="floor"):
        dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 3, floor=("snap", 6, 0))


def test_command_line(world):
    """`main.py --infer --dense --stride 3 --floor clamp --save_pred ...` in a fresh child process on the tree as it lies on disk (the
    floor is z = 1 seen from above, h = 1 - z, so a margin of 80 cm raises every leg that reaches above z = 0.2): the new lines behind the existing ones, the new arrays and scalars in
    the file; a run without --floor writes exactly today's key set."""
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=str(world.tmp / "train_out"))
    head = [sys.executable, os.path.join(ROOT, "main.py"), "--infer", "--dense", "--stride", "3", "--gt_head_pose", "--data_root", world.data,
            "--device", "cuda:0", "--seed", "3", "--batch_size", "4", "--load_Upper_path", str(world.tmp / "upper.pth"), "--load_Lower_path",
            str(world.tmp / "lower.pth")]
    path, plain = str(world.tmp / "pred.npz"), str(world.tmp / "plain.npz")
    r = subprocess.run(head + ["--save_pred", path, "--floor", "clamp", "--floor_margin_cm", "80"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    out = r.stdout
    lines = ["Average Joint Localization Error(cm):", "Average UpperBody Joint Localization Error(cm):",
             "Average LowerBody Joint Localization Error(cm):", "Average Joint Rotation Error", "Per Joint Localization Error(cm):",
             "Single-window (unblended) Error(cm):", "Dense windows:", "Per-frame skeletons saved in", "Foot Height Error(cm): ",
             "Floor Penetration: rate ", "Foot Contact by height < 6 cm: precision ", "Contact Hover(cm): ", "Unclamped Error(cm): all ",
             "Floor Clamp: "]
    at = [out.index(line) for line in lines]
    assert at == sorted(at), "the lines come in this order"
    assert " of 84 frames lifted, mean lift(cm) " in out and "(margin 80 cm)" in out
    z = np.load(path)
    today = {"pred", "covered", "spread", "recording", "frame_in_recording", "target", "stride", "blend", "frame_no"}
    assert set(z.files) == today | {"foot_height", "ground", "foot_contact", "floor_mode", "floor_contact_cm", "floor_margin_cm",
                                    "pred_unclamped", "lifted", "floor_fallback"}
    assert str(z["floor_mode"]) == "clamp" and float(z["floor_contact_cm"]) == 6.0 and float(z["floor_margin_cm"]) == 80.0
    for k, shape in (("foot_height", (F, 2)), ("ground", (F, 4)), ("foot_contact", (F, 2)), ("pred_unclamped", (F, 21, 3)), ("lifted", (F,)),
                     ("floor_fallback", (F,)), ("pred", (F, 21, 3))):
        assert z[k].shape == shape, k
    assert np.array_equal(z["ground"], np.tile(np.float32([0, 0, -1, 1]), (F, 1))) and np.array_equal(z["foot_contact"], np.tile(np.float32([1, 0]), (F, 1)))
    cov = z["covered"] > 0
    reached = cov & (z["floor_fallback"] == 0)
    assert (z["lifted"][cov] > 0).any() and not z["lifted"][~cov].any() and reached.any()
    assert (z["foot_height"][reached] >= np.float32(0.8)).all() and np.isnan(z["foot_height"][~cov]).all()
    still = cov & (z["lifted"] == 0)
    assert z["pred"][still].tobytes() == z["pred_unclamped"][still].tobytes()
    r = subprocess.run(head + ["--save_pred", plain], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    assert "Floor" not in r.stdout and "Foot" not in r.stdout
    zp = np.load(plain)
    assert set(zp.files) == today and zp["pred"].tobytes() == z["pred_unclamped"].tobytes()
