"""CPU: the host side of the renderer (mmego_amd/render.py) and its command line -- the camera on built frames, the animated-PNG writer
against the reader of tests/render_ref.py, the parser's refusals by their messages -- and the cap on the float64 restatement alone: run
in float32 on the raster test's own inputs it moves no channel by more than one level, and at most 0.5 % of them at all."""
import numpy as np
import pytest

import main as cli
import render_ref as ref
from mmego_amd import ops, render, skeleton


def _frames():
    """Three standing frames over the plane z = 0, hips along +x; frame 1 shifted, frame 2 with a plane of zero normal."""
    t = np.zeros((3, 21, 3))
    t[:, :, 2] = np.linspace(0.1, 1.7, 21)
    t[:, :, 0] = np.linspace(-0.2, 0.2, 21)
    t[:, 12], t[:, 16], t[:, 0], t[:, 20] = [-0.15, 0.02, 0.9], [0.15, 0.02, 0.9], [0.01, 0.03, 1.0], [0.01, 0.03, 1.7]
    t[1] += [0.5, -0.3, 0.0]
    g = np.tile([0.0, 0.0, 2.0, 0.0], (3, 1))
    g[2] = 0.0
    return t, g


def test_camera_centres_joint_0_and_front_is_x_minus_z():
    t, g = _frames()
    for view in render.VIEWS:
        cam = render.camera(t, g, view, 256)
        assert cam.shape == (3, 8) and cam.dtype == np.float32
        M = cam.astype(np.float64).reshape(3, 2, 4)
        centre = np.einsum("fij,fj->fi", M[:, :, :3], t[:, 0]) + M[:, :, 3]
        assert np.abs(centre - 128.0).max() <= 1e-4
        assert np.abs(cam - ref.camera(t, g, view, 256)).max() <= 1e-4
    s = 256 / 2.4
    front = render.camera(t, g, "front", 256).astype(np.float64)
    for f in (0, 1, 2):                                            # (frame 2: no plane, up is t20 - t0 = +z as well)
        assert np.abs(front[f, :3] - [s, 0, 0]).max() <= 1e-4 and np.abs(front[f, 4:7] - [0, 0, -s]).max() <= 1e-4
    side = render.camera(t, g, "side", 256).astype(np.float64)
    assert np.abs(side[0, :3] - [0, s, 0]).max() <= 1e-4 and np.abs(side[0, 4:7] - [0, 0, -s]).max() <= 1e-4     # (up x l = z x x = y)
    # hips on the vertical: the left-right axis falls back to the ring's e1
    t[0, 16] = t[0, 12] + [0.0, 0.0, 0.3]
    cam = render.camera(t, g, "front", 64).astype(np.float64)
    assert np.abs(cam[0, :3] - [64 / 2.4, 0, 0]).max() <= 1e-5
    assert np.abs(cam - ref.camera(t, g, "front", 64)).max() <= 1e-4
    with pytest.raises(ValueError, match="view"):
        render.camera(t, g, "top", 64)


def test_ring_table_and_bones_are_the_restatements():
    assert np.array_equal(ops.RENDER_RING, ref.RING) and ops.RENDER_RING.dtype == np.float32
    assert ops.RENDER_FIXED == 32 + 3 * len(skeleton.BONES_ALL) + 2 * 21 == 134
    c = ref.scene_case()
    P = ref.prims_of(c["pred"], c["tgt"], c["ground"], c["cloud"], c["seg"], ref.camera(c["tgt"], c["ground"], "front", 64), 1.0)
    assert P.shape == (5, 141, 12)


def test_apng_round_trip(tmp_path):
    frames = np.random.default_rng(0).integers(0, 256, (3, 16, 20, 3)).astype(np.uint8)
    path = render.write_apng(str(tmp_path / "a.png"), frames, 25)
    got, delay = ref.read_apng(path)
    assert got.dtype == np.uint8 and got.shape == frames.shape and got.tobytes() == frames.tobytes()
    assert delay == (1, 25)
    one, _ = ref.read_apng(render.write_apng(str(tmp_path / "b.png"), frames[:1], 1))
    assert one.tobytes() == frames[:1].tobytes()
    for bad, fps in ((frames.astype(np.int32), 10), (frames[0], 10), (frames, 0), (frames, 101), (frames, 2.5)):
        with pytest.raises(ValueError, match="write_apng"):
            render.write_apng(str(tmp_path / "c.png"), bad, fps)


def _refused(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_parser_refusals(capsys, monkeypatch):
    dense = ["--infer", "--dense"]
    for flag, value in (("--render", "d"), ("--render_size", "64"), ("--render_recordings", "0"), ("--render_fps", "5")):
        assert "%s belongs to --infer --dense" % flag in _refused(["--infer", flag, value], capsys, monkeypatch)
    for flag, value in (("--render_size", "64"), ("--render_recordings", "0"), ("--render_fps", "5")):
        assert "%s belongs to --render DIR" % flag in _refused(dense + [flag, value], capsys, monkeypatch)
    for size in ("60", "1028", "66", "-4"):
        assert "--render_size is a view's edge in pixels" in _refused(dense + ["--render", "d", "--render_size", size], capsys, monkeypatch)
    for recs in ("", "a", "1,,2", "-1", "1.5", "0,x", "1, 2", "\u00b2", "\u0663"):
        assert "--render_recordings is a comma-separated list" in _refused(dense + ["--render", "d", "--render_recordings=" + recs], capsys, monkeypatch)
    for fps in ("0", "101", "-3"):
        assert "--render_fps is the animation's frames per second" in _refused(dense + ["--render", "d", "--render_fps", fps], capsys, monkeypatch)
    assert "--render does not go with --vis" in _refused(["--infer", "--vis", "--render", "d"], capsys, monkeypatch)
    assert "--render does not go with --vis" in _refused(dense + ["--vis", "--render", "d"], capsys, monkeypatch)
    assert "--dense does not go with --vis" in _refused(dense + ["--vis"], capsys, monkeypatch)


def test_parser_accepts_and_fills_the_config(monkeypatch):
    p = cli.build_parser()
    args = p.parse_args(["--infer", "--dense", "--render", "out", "--render_recordings", "3,0,7", "--render_size", "64"])
    cli.check_render(p, args)
    assert cli.parse_recordings(args.render_recordings) == [3, 0, 7]
    from mmego_amd import config, dense
    assert dense._check_render(("out", 64, [3, 0, 7, 3], 10)) == ("out", 64, (0, 3, 7), 10)
    assert dense._check_render(None) is None and (config.RENDER_SIZE, config.RENDER_FPS) == (256, 10)
    for bad in (("out", 62, None, 10), ("out", 64, [], 10), ("out", 64, [-1], 10), ("out", 64, None, 0), ("", 64, None, 10), ("out", 64, None)):
        with pytest.raises(ValueError, match="render"):
            dense._check_render(bad)


def test_reference_in_float32_is_within_one_level_of_float64():
    """The cap on the reference alone, on the GPU raster test's inputs: the compositing is continuous, so float32 can only flip the
    final rounding -- no channel differs by more than 1 level, and at most 0.5 % of the channels differ at all."""
    diff = total = 0
    for I, W, H, P, tables in ref.raster_cases():
        for i in range(I):
            a = ref.raster(tables[i], W, H, (255, 250, 240), np.float64).astype(np.int32)
            b = ref.raster(tables[i], W, H, (255, 250, 240), np.float32).astype(np.int32)
            assert np.abs(a - b).max() <= 1, (W, H, P, i)
            diff, total = diff + int((a != b).sum()), total + a.size
    print("float32 against float64: %d of %d channel values differ (%.4f %%)" % (diff, total, 100.0 * diff / total))
    assert diff <= 0.005 * total
