"""GPU: the renderer (csrc/render.hip through ops.render_raster / ops.render_prims, mmego_amd/render.py, dense_infer's render=, the
command line) against the float64 restatement of tests/render_ref.py.

The bars.  Raster: the composite is continuous in every input and the kernel's cull is conservative beyond the roundings of the distance (a culled primitive covers nothing), so
against float64 only the final rounding can flip -- every channel within 1 level, differing values at most 0.5 % of all (the float32
run of the restatement itself stays inside the same bar: tests/test_render_cpu.py).  Scene: the kernel computes in double and rounds
once, the bars are the issue's derived ones for an all-float32 kernel -- coordinates within 2e-3 px (values up to 512, an ulp of 6e-5,
a dozen roundings), colours within 1e-3 level, radii and alphas exact, absent records all zero."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as ref
import test_dense_infer_gpu as di
from conftest import ROOT

pytestmark = pytest.mark.gpu

BG = (255, 250, 240)
SENTINEL = 77


def _raster_bar(got, want, what):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((d != 0).mean())
    print("%s: %d of %d channel values differ from float64 (%.4f %%), largest difference %d" % (what, int((d != 0).sum()), d.size,
                                                                                               100.0 * share, int(d.max())))
    assert d.max() <= 1, what
    assert share <= 0.005, what
    return share


@pytest.fixture(scope="module")
def raster_refs():
    """The float64 images of every raster case, computed once."""
    return [(I, W, H, P, t, np.stack([ref.raster(t[i], W, H, BG) for i in range(I)])) for I, W, H, P, t in ref.raster_cases()]


def _frame_and_view(I, W, H, dev):
    """A sentinel-filled frame and the W x H viewport inside it: 36 x 20 one row down and four pixels in, 64 x 64 at column 64 of 128."""
    if W == 64:
        frame = torch.full((I, 64, 128, 3), SENTINEL, dtype=torch.uint8, device=dev)
        return frame, frame[:, :, 64:128], (slice(None), slice(None), slice(64, 128))
    frame = torch.full((I, H + 2, W + 4, 3), SENTINEL, dtype=torch.uint8, device=dev)
    return frame, frame[:, 1:H + 1, 4:W + 4], (slice(None), slice(1, H + 1), slice(4, W + 4))


def test_raster_against_the_reference(raster_refs):
    from mmego_amd import ops
    dev = torch.device("cuda")
    for I, W, H, P, tables, want in raster_refs:
        prims = torch.as_tensor(tables).to(dev)
        frame, view, where = _frame_and_view(I, W, H, dev)
        ops.render_raster(prims, view, BG)
        first = frame.cpu().numpy()
        _raster_bar(first[where], want, "raster I=%d %dx%d P=%d" % (I, W, H, P))
        outside = np.ones(first.shape, dtype=bool)
        outside[where] = False
        assert (first[outside] == SENTINEL).all(), "bytes outside the viewport were written"
        if P == 0:
            assert (first[where] == np.asarray(BG, dtype=np.uint8)).all()
        ops.render_raster(prims, view, BG)                         # a second launch: the same bytes
        assert frame.cpu().numpy().tobytes() == first.tobytes()
        if P == 64:                                                # the order is honoured: image 0 reversed is another image
            rev = prims.clone()
            rev[0] = prims[0].flip(0)
            ops.render_raster(rev, view, BG)
            again = frame.cpu().numpy()
            assert (again[where][0] != first[where][0]).any()
            _raster_bar(again[where][0], ref.raster(tables[0][::-1], W, H, BG), "reversed")
            assert again[where][1:].tobytes() == first[where][1:].tobytes()


@pytest.fixture(scope="module")
def scene():
    c = ref.scene_case()
    c["cam"] = np.stack([ref.camera(c["tgt"], c["ground"], v, 512).astype(np.float32)[f] for f, v in enumerate(("front", "side", "front", "side", "front"))])
    c["want"] = ref.prims_of(c["pred"], c["tgt"], c["ground"], c["cloud"], c["seg"], c["cam"], 0.8)
    return c


def test_scene_against_the_reference(scene):
    from mmego_amd import ops
    dev = torch.device("cuda")
    d = {k: torch.as_tensor(scene[k]).to(dev) for k in ("pred", "tgt", "ground", "cloud", "seg", "cam")}
    F, N = 5, 7
    # row strides beyond 63: the frames as columns of wider tables
    wide_p, wide_t = torch.zeros((F, 70), device=dev), torch.zeros((F, 64), device=dev)
    wide_p[:, :63], wide_t[:, :63] = d["pred"], d["tgt"]
    prims = torch.full((F, 134 + N, 12), 9.0, device=dev)
    ops.render_prims(wide_p[:, :63], wide_t[:, :63], d["ground"], d["cloud"], d["seg"], d["cam"], 0.8, prims)
    got, want = prims.cpu().numpy().astype(np.float64), scene["want"]
    assert np.abs(want[:, :, :4]).max() <= 1024 and np.isfinite(got).all()
    coord, colour = np.abs(got[:, :, :4] - want[:, :, :4]).max(), np.abs(got[:, :, 6:9] - want[:, :, 6:9]).max()
    print("scene: coordinates within %.3g px, colours within %.3g level" % (coord, colour))
    assert coord <= 2e-3 and colour <= 1e-3
    # (exact: the float32 of the recipe's radius and alpha, 0.35 and 0.8 among them)
    assert np.array_equal(got[:, :, 4:6], want[:, :, 4:6].astype(np.float32).astype(np.float64)) and (got[:, :, 9:] == 0).all()
    absent = (want == 0).all(axis=2)
    assert (got[absent] == 0).all() and (got[~absent][:, 5] > 0).all()
    # what is absent where: frame 1 (seg < 0) shadow, predicted bones and joints; frame 2 (no plane) ring and shadow; frame 3 two returns
    assert absent[1, 32:52].all() and absent[1, 93 + N:].all() and not absent[1, :32].any() and not absent[1, 52:93 + N].any()
    assert absent[2, :52].all() and not absent[2, 52:].any()
    assert list(np.flatnonzero(absent[3])) == [93 + 2, 93 + 6] and not absent[0].any() and not absent[4].any()
    again = torch.empty_like(prims)
    ops.render_prims(d["pred"], d["tgt"], d["ground"], d["cloud"], scene["seg"], d["cam"], 0.8, again)      # (seg as a host array)
    assert torch.equal(again, prims)
    # N = 0: the 134 fixed records, the same as above around the cloud
    bare = torch.empty((F, 134, 12), device=dev)
    ops.render_prims(d["pred"], d["tgt"], d["ground"], d["cloud"][:, :0].contiguous(), d["seg"], d["cam"], 0.8, bare)
    assert torch.equal(bare[:, :93], prims[:, :93]) and torch.equal(bare[:, 93:], prims[:, 93 + N:])


def test_refusals_launch_nothing(scene, monkeypatch):
    from mmego_amd import hip, ops
    dev = torch.device("cuda")
    d = {k: torch.as_tensor(scene[k]).to(dev) for k in ("pred", "tgt", "ground", "cloud", "seg", "cam")}
    prims = torch.zeros((5, 141, 12), device=dev)
    out = torch.zeros((5, 32, 64, 3), dtype=torch.uint8, device=dev)
    raw = torch.zeros(5 * 32 * 64 * 3 + 64, dtype=torch.uint8, device=dev)
    launched = []
    monkeypatch.setattr(hip, "_launch", lambda name, *a: launched.append(name))
    ok = dict(pred=d["pred"], tgt=d["tgt"], ground=d["ground"], cloud=d["cloud"], seg=d["seg"], cam=d["cam"], vmax=1.0, prims=prims)
    ops.render_prims(**ok)
    ops.render_raster(prims, out)
    assert launched == ["render_prims", "render_raster"]
    del launched[:]
    f32 = lambda *s: torch.zeros(s, device=dev)
    for change in (dict(pred=None), dict(tgt=None), dict(ground=None), dict(cloud=None), dict(cam=None), dict(prims=None), dict(seg=None),
                   dict(pred=d["pred"][:, :62]), dict(tgt=d["tgt"][:, :60]), dict(tgt=d["tgt"][:4]), dict(ground=f32(5, 3)), dict(cam=f32(5, 7)),
                   dict(cloud=f32(5, 891, 6), prims=f32(5, 1025, 12)), dict(cloud=f32(5, 7, 5)), dict(cloud=d["cloud"].cpu()),
                   dict(seg=d["seg"].to(torch.int64)), dict(seg=scene["seg"][:4]), dict(vmax=0.0), dict(vmax=-1.0), dict(vmax=float("nan")),
                   dict(vmax=float("inf")), dict(prims=f32(5, 140, 12)), dict(prims=f32(5 * 141 * 12 + 1)[1:].view(5, 141, 12)),
                   dict(prims=prims.to(torch.float64)), dict(pred=d["pred"].to(torch.float64))):
        with pytest.raises(ValueError, match="render_prims"):
            ops.render_prims(**dict(ok, **change))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
    for p, o, bg in ((None, out, BG), (prims, None, BG), (f32(0, 141, 12), u8(0, 32, 64, 3), BG), (f32(5, 1025, 12), out, BG),
                     (f32(5, 141, 11), out, BG), (f32(5 * 141 * 12 + 1)[1:].view(5, 141, 12), out, BG), (prims, u8(4, 32, 64, 3), BG),
                     (prims, u8(5, 12, 64, 3), BG), (prims, u8(5, 2052, 16, 3), BG), (prims, u8(5, 32, 12, 3), BG), (prims, u8(5, 16, 2052, 3), BG),
                     (prims, u8(5, 32, 18, 3), BG),                                  # W % 4
                     (prims, u8(5, 32, 64, 4), BG), (prims, out.float(), BG), (prims, out.cpu(), BG),
                     (prims, u8(5, 32, 66, 3)[:, :, :64], BG),                       # a pitch of 198 bytes: no multiple of 4
                     (prims, u8(5, 33, 68, 3)[:, :32, 1:65], BG),                   # out 3 bytes in: not 4-byte aligned
                     (prims, raw[:5 * 6146].view(5, 6146)[:, :6144].view(5, 32, 64, 3), BG),      # an image stride of 6146: no multiple of 4
                     (prims, u8(5, 32, 64, 6)[:, :, :, :3], BG),                     # pixels 6 bytes apart
                     (prims, out, (256, 0, 0)), (prims, out, (0, -1, 0)), (prims, out, (0, 0)), (prims, out, (1.5, 0, 0))):
        with pytest.raises(ValueError, match="render_raster"):
            ops.render_raster(p, o, bg)
    assert launched == []
    monkeypatch.undo()
    # the C ABI itself answers -1 (and returns ahead of its launch) for the same
    lib, s = hip.lib(), hip.stream_handle()
    P, O = prims.data_ptr(), out.data_ptr()
    good = [s, P, 5, 141, O, 64, 32, 192, 32 * 192, 255, 255, 255]
    for i, v in ((1, None), (4, None), (2, 0), (3, -1), (3, 1025), (5, 12), (5, 2052), (5, 62), (6, 15), (6, 2049), (7, 188), (7, 194), (8, 32 * 192 - 4),
                 (8, 32 * 192 + 2), (4, O + 2), (1, P + 4), (9, 256), (10, -1), (11, 300)):
        bad = list(good)
        bad[i] = v
        assert lib.mmego_render_raster(*bad) == -1, (i, v)
    ring = ops._upload_once(dev, ops.RENDER_RING)[0].data_ptr()
    ptr = {k: d[k].data_ptr() for k in d}
    good = [s, ptr["pred"], 63, ptr["tgt"], 63, ptr["ground"], ptr["cloud"], 7, ptr["seg"], ptr["cam"], ring, 5, 1.0, P]
    for i, v in ((1, None), (3, None), (5, None), (6, None), (8, None), (9, None), (10, None), (13, None), (11, 0), (11, 2 ** 31), (7, -1), (7, 891),
                 (2, 62), (4, 62), (12, 0.0), (12, float("nan")), (12, float("inf")), (13, P + 4)):
        bad = list(good)
        bad[i] = v
        assert lib.mmego_render_prims(*bad) == -1, (i, v)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """test_dense_infer_gpu's synthetic tree (recordings of 23, 20, 7 and 41 frames, T = 20), seeded nets, and the pass with and
    without render."""
    from mmego_amd import dense, nets, processors
    from mmego_amd.config import ConfigDemo
    from mmego_amd.data import PosePC
    w = di._World()
    w.tmp = tmp_path_factory.mktemp("render")
    w.data = str(w.tmp / "Sample_data")
    di._make_dataset(w.data, np.random.default_rng(0))
    np.random.seed(3)
    w.ds = PosePC(train=False, vis=True, keep_frames=True, batch_length=di.T, root=w.data)
    keep = ConfigDemo.gt_head_pose
    ConfigDemo.gt_head_pose = True
    try:
        w.base = processors._Base(ConfigDemo, make_dirs=False)
    finally:
        ConfigDemo.gt_head_pose = keep
    torch.manual_seed(0)
    w.up, w.lo = nets.UpperNet().to(w.base.device).eval(), nets.LowerNet(64).to(w.base.device).eval()
    torch.save(w.up.state_dict(), w.tmp / "upper.pth")
    torch.save(w.lo.state_dict(), w.tmp / "lower.pth")
    w.dir = str(w.tmp / "pictures")
    kw = dict(blend="triangle", batch_size=4, smooth=(2, 1, "gauss"), floor=("clamp", 6.0, 1.0))
    w.plain = dense.dense_infer(w.base, None, w.up, w.lo, w.ds, 5, **kw)
    w.drawn = dense.dense_infer(w.base, None, w.up, w.lo, w.ds, 5, render=(w.dir, 64, None, 10), **kw)
    return w


def test_the_pass_writes_one_file_per_covered_recording(world):
    s, a = world.drawn
    assert sorted(os.listdir(world.dir)) == ["rec0000_action1.png", "rec0001_action2.png", "rec0003_action2.png"]
    assert s["rendered_recordings"] == 3 and s["rendered_frames"] == 23 + 20 + 41
    plan = a["plan"]
    cloud = plan.src["data"].cpu().numpy().reshape(di.F, -1, 6)
    ground = np.asarray(world.ds.frame_ground_, dtype=np.float32)
    seg = np.where(a["covered"] != 0, a["recording"], -1).astype(np.int32)
    pred = np.nan_to_num(a["pred"].reshape(di.F, 63))
    share = []
    for name, rec, n in (("rec0000_action1.png", 0, 23), ("rec0001_action2.png", 1, 20), ("rec0003_action2.png", 3, 41)):
        frames, delay = ref.read_apng(os.path.join(world.dir, name))
        assert frames.shape == (n, 64, 128, 3) and delay == (1, 10)
        rows = np.flatnonzero(a["recording"] == rec)               # every frame of the recording, in order
        assert len(rows) == n
        want = ref.render_frames(pred[rows], a["target"].reshape(di.F, 63)[rows], ground[rows], cloud[rows], seg[rows], 64)
        share.append(_raster_bar(frames, want, name))
        assert (frames != 255).any(axis=(1, 2, 3)).all()           # no frame is blank
    # the pictures are of the FINAL frames: pred is behind the filter and the clamp, and differs from the blend
    assert not np.array_equal(a["pred"], a["pred_unsmoothed"], equal_nan=True)


def test_a_loader_without_planes_is_refused_ahead_of_the_pass(world, monkeypatch):
    from mmego_amd import dense
    monkeypatch.setattr(world.ds, "frame_ground_", None)
    ran = []
    monkeypatch.setattr(dense, "_dense_pass", lambda *a, **k: ran.append(1))
    with pytest.raises(ValueError, match="frame_ground_"):
        dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 5, render=(str(world.tmp / "never"), 64, None, 10))
    assert not ran and not os.path.exists(str(world.tmp / "never"))
    with pytest.raises(ValueError, match="recording 4 is not one of the loader's 4"):
        monkeypatch.undo()
        dense.dense_infer(world.base, None, world.up, world.lo, world.ds, 5, render=(str(world.tmp / "never"), 64, [0, 4], 10))


def test_render_frames_in_more_than_one_chunk(scene, monkeypatch):
    """render_frames with its chunk at 2 frames (three rounds for 5 frames, the last one short) gives the bytes of the single round."""
    from mmego_amd import render
    dev = torch.device("cuda")
    d = {k: torch.as_tensor(scene[k]).to(dev) for k in ("pred", "tgt", "ground", "cloud", "seg")}
    whole = render.render_frames(d["pred"], d["tgt"], d["ground"], d["cloud"], d["seg"], 64, vmax=0.8).cpu().numpy()
    monkeypatch.setattr(render, "CHUNK", 2)
    parts = render.render_frames(d["pred"], d["tgt"], d["ground"], d["cloud"], d["seg"], 64, vmax=0.8).cpu().numpy()
    assert parts.shape == (5, 64, 128, 3) and parts.tobytes() == whole.tobytes()
    want = ref.render_frames(scene["pred"], scene["tgt"], scene["ground"], scene["cloud"], scene["seg"], 64, vmax=0.8)
    _raster_bar(parts, want, "five frames in chunks of two")
    assert len({parts[f].tobytes() for f in range(5)}) == 5      # (five different frames: an offset mistake would repeat one)


def _same(x, y):
    if isinstance(x, dict):
        return isinstance(y, dict) and set(x) == set(y) and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, (tuple, list)):
        return type(x) is type(y) and len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    if isinstance(x, np.ndarray):
        return isinstance(y, np.ndarray) and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    return x == y or (isinstance(x, float) and isinstance(y, float) and np.isnan(x) and np.isnan(y))


def test_render_leaves_the_pass_alone(world):
    (s0, a0), (s1, a1) = world.plain, world.drawn
    assert set(s1) - set(s0) == {"rendered_recordings", "rendered_frames"} and set(a0) == set(a1)
    for k in s0:
        assert _same(s0[k], s1[k]), k
    for k in a0:
        if isinstance(a0[k], torch.Tensor):
            assert torch.equal(a0[k], a1[k]), k
        elif isinstance(a0[k], np.ndarray):
            assert a0[k].tobytes() == a1[k].tobytes(), k


def test_an_uncovered_frame_shows_the_target_alone(world):
    """render_frames on the 7-frame recording (seg < 0 everywhere) is the picture of the same frames without any prediction."""
    from mmego_amd import render
    s, a = world.drawn
    plan, dev = a["plan"], world.base.device
    rows = np.flatnonzero(a["recording"] == 2)
    assert len(rows) == 7 and (a["covered"][rows] == 0).all()
    lo, hi = int(rows[0]), int(rows[-1]) + 1
    tgt, ground = plan.src["target"][lo:hi], plan.floor()[0][lo:hi]
    cloud = plan.src["data"].view(di.F, -1, 6)[lo:hi]
    img = render.render_frames(torch.zeros((7, 63), device=dev), tgt, ground, cloud, np.full(7, -1, dtype=np.int32), 64).cpu().numpy()
    want = ref.render_frames(np.zeros((2, 63)), tgt.cpu().numpy()[:2], ground.cpu().numpy()[:2], cloud.cpu().numpy()[:2], np.array([-1, -1]), 64)
    _raster_bar(img[:2], want, "uncovered frames")
    # and whatever the prediction's rows hold there is not looked at
    junk = torch.as_tensor(np.random.default_rng(1).normal(0.5, 0.5, (7, 63)).astype(np.float32)).to(dev)
    other = render.render_frames(junk, tgt, ground, cloud, np.full(7, -1, dtype=np.int32), 64).cpu().numpy()
    assert other.tobytes() == img.tobytes()
    shown = render.render_frames(junk, tgt, ground, cloud, np.zeros(7, dtype=np.int32), 64).cpu().numpy()
    assert (shown != img).any(axis=(1, 2, 3)).all()                # (with seg >= 0 the same rows are drawn)


def _main(args, env, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_command_line(world):
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=str(world.tmp / "train_out"))
    common = ["--gt_head_pose", "--data_root", world.data, "--device", "cuda:0", "--seed", "3", "--load_Upper_path", str(world.tmp / "upper.pth"),
              "--load_Lower_path", str(world.tmp / "lower.pth")]
    out_dir = str(world.tmp / "cli")
    out = _main(["--infer", "--dense", "--render", out_dir, "--render_recordings", "0", "--render_size", "64", "--batch_size", "4"] + common, env, ROOT)
    assert os.listdir(out_dir) == ["rec0000_action1.png"]
    assert "Rendered: 1 recordings, 23 frames -> %s" % out_dir in out
    frames, _ = ref.read_apng(os.path.join(out_dir, "rec0000_action1.png"))
    assert frames.shape == (23, 64, 128, 3)
    cwd = str(world.tmp / "cwd")
    os.makedirs(cwd)
    out = _main(["--infer", "--vis"] + common, env, cwd)
    vis = os.path.join(cwd, "vis", "1")
    assert sorted(os.listdir(vis)) == ["rec0000_action1.png", "rec0001_action2.png", "rec0003_action2.png"]
    assert "Dense windows: 6 windows of 20 frames at stride 20 (blend mean), 84 of 91 frames covered, largest cover 2" in out
    assert "Rendered: 3 recordings, 84 frames -> " in out and "Average Joint Localization Error(cm):" in out
    frames, delay = ref.read_apng(os.path.join(vis, "rec0003_action2.png"))
    assert frames.shape == (41, 256, 512, 3) and delay == (1, 10)
