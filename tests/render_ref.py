"""Float64 numpy restatement of the renderer (csrc/render.hip, the recipe in include/mmego_hip.h; mmego_amd/render.py): the compositor
raster(), the scene prims_of(), the camera, and a reader for the animated PNGs render.write_apng writes (filter type 0 only).  Written
from the recipe, frame by frame and primitive by primitive, sharing no code with the product."""
import struct
import zlib

import numpy as np

from mmego_amd import skeleton

RING = np.stack([np.cos(2.0 * np.pi * np.arange(32) / 32.0), np.sin(2.0 * np.pi * np.arange(32) / 32.0)], axis=1).astype(np.float32)
F32_MAX = float(np.finfo(np.float32).max)


def contributes(rec):
    """The recipe's rule for one record (12 floats as the device holds them, float32)."""
    rec = np.asarray(rec, dtype=np.float32)
    if not np.isfinite(rec[:9]).all() or not rec[5] > 0 or not rec[4] >= 0:
        return False
    d = rec[2:4].astype(np.float64) - rec[0:2].astype(np.float64)
    return float(d @ d) <= F32_MAX                                  # (|b - a|^2 fits fp32)


def raster(prims, W, H, bg, dtype=np.float64):
    """One image [H, W, 3] uint8 of the table prims [P, 12], every operation in ``dtype``."""
    prims = np.asarray(prims, dtype=np.float32)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px, py = (xs + 0.5).astype(dtype), (ys + 0.5).astype(dtype)
    col = np.empty((H, W, 3), dtype=dtype)
    col[:] = np.asarray(bg, dtype=dtype)
    zero, one, half = dtype(0), dtype(1), dtype(0.5)
    for rec in prims:
        if not contributes(rec):
            continue
        ax, ay, bx, by, r, alpha = (dtype(v) for v in rec[:6])
        dx, dy = bx - ax, by - ay
        l2 = dx * dx + dy * dy
        if l2 > 0:
            t = np.clip(((px - ax) * dx + (py - ay) * dy) / l2, zero, one)
        else:
            t = np.zeros_like(px)
        d = np.sqrt((px - (ax + t * dx)) ** 2 + (py - (ay + t * dy)) ** 2)
        c = np.clip(r + half - d, zero, one) * alpha
        col += c[:, :, None] * (rec[6:9].astype(dtype) - col)
    return (np.clip(col, zero, dtype(255)) + half).astype(np.int32).astype(np.uint8)


def _plane(g):
    n = np.linalg.norm(g[:3])
    return (g[:3] / n, g[3] / n) if n > 1e-6 else None


def ring_axes(u):
    ax = int(np.argmin(np.abs(u)))                                  # (the first on ties)
    e = np.eye(3)[ax]
    w = e - (e @ u) * u
    e1 = w / np.linalg.norm(w)
    return e1, np.cross(u, e1)


def _error_colour(e):
    s = min(e / 0.15, 1.0)
    return np.array([0.0, 170.0, 0.0]) + s * (np.array([230.0, 0.0, 0.0]) - np.array([0.0, 170.0, 0.0]))


def prims_of(pred, tgt, ground, cloud, seg, cam, vmax):
    """The scene [F, 134 + N, 12] in float64 from host arrays: pred, tgt [F, 63], ground [F, 4], cloud [F, N, 6], seg [F], cam [F, 8]."""
    pred, tgt = np.asarray(pred, dtype=np.float64).reshape(-1, 21, 3), np.asarray(tgt, dtype=np.float64).reshape(-1, 21, 3)
    ground, cloud, cam = np.asarray(ground, dtype=np.float64), np.asarray(cloud, dtype=np.float64), np.asarray(cam, dtype=np.float64)
    F, N = len(pred), cloud.shape[1]
    out = np.zeros((F, 134 + N, 12))
    for f in range(F):
        M, o = cam[f].reshape(2, 4), cam[f].reshape(2, 4)[:, 3]
        proj = lambda x: M[:, :3] @ x + o
        rows = []

        def put(a, b, r, alpha, colour):
            rows.append(np.concatenate([proj(a), proj(b), [r, alpha], colour, [0.0, 0.0, 0.0]]))

        absent = lambda n=1: rows.extend([np.zeros(12)] * n)
        plane, has = _plane(ground[f]), seg[f] >= 0
        if plane is None:
            absent(32)
        else:
            u, d = plane
            drop = lambda x: x - (u @ x + d) * u
            foot, (e1, e2) = drop(tgt[f, 0]), ring_axes(u)
            vert = [foot + float(RING[k, 0]) * e1 + float(RING[k, 1]) * e2 for k in range(32)]
            for k in range(32):
                put(vert[k], vert[(k + 1) % 32], 0.5, 1.0, [170.0] * 3)
        for p, c in skeleton.BONES_ALL:
            if plane is None or not has:
                absent()
            else:
                put(drop(pred[f, p]), drop(pred[f, c]), 2.0, 0.35, [60.0] * 3)
        for p, c in skeleton.BONES_ALL:
            put(tgt[f, p], tgt[f, c], 1.5, 1.0, [120.0] * 3)
        for j in range(21):
            put(tgt[f, j], tgt[f, j], 2.5, 1.0, [90.0] * 3)
        for row in cloud[f]:
            if (row[:3] == 0).all():
                absent()
                continue
            s = min(max(0.5 + row[4] / (2.0 * vmax), 0.0), 1.0)
            put(row[:3], row[:3], 1.5, 0.8, np.array([40.0, 90.0, 220.0]) + s * (np.array([230.0, 60.0, 40.0]) - np.array([40.0, 90.0, 220.0])))
        for p, c in skeleton.BONES_ALL:
            if has:
                put(pred[f, p], pred[f, c], 2.0, 1.0, _error_colour(np.linalg.norm(pred[f, c] - tgt[f, c])))
            else:
                absent()
        for j in range(21):
            if has:
                put(pred[f, j], pred[f, j], 3.0, 1.0, _error_colour(np.linalg.norm(pred[f, j] - tgt[f, j])))
            else:
                absent()
        out[f] = np.stack(rows)
    return out


def camera(target, ground, view, size, metres=2.4):
    """cam [F, 8] in float64, frame by frame."""
    target, ground = np.asarray(target, dtype=np.float64).reshape(-1, 21, 3), np.asarray(ground, dtype=np.float64)
    cams = []
    for t, g in zip(target, ground):
        plane = _plane(g)
        up = plane[0] if plane is not None else (t[20] - t[0]) / np.linalg.norm(t[20] - t[0])
        hips = t[16] - t[12]
        l = hips - (hips @ up) * up
        l = l / np.linalg.norm(l) if np.linalg.norm(l) >= 1e-6 else ring_axes(up)[0]
        right = l if view == "front" else np.cross(up, l)
        s = size / metres
        cams.append(np.concatenate([s * right, [size / 2.0 - s * (right @ t[0])], -s * up, [size / 2.0 + s * (up @ t[0])]]))
    return np.asarray(cams)


def render_frames(pred, tgt, ground, cloud, seg, size, vmax=1.0, dtype=np.float64):
    """[F, size, 2 size, 3] uint8: front view left, side view right, on a white background; the cameras rounded to float32 as the
    device receives them."""
    F = len(pred)
    out = np.empty((F, size, 2 * size, 3), dtype=np.uint8)
    for v, view in enumerate(("front", "side")):
        cam = camera(tgt, ground, view, size).astype(np.float32)
        P = prims_of(pred, tgt, ground, cloud, seg, cam, vmax)
        for f in range(F):
            out[f, :, v * size:(v + 1) * size] = raster(P[f].astype(np.float32), size, size, (255, 255, 255), dtype)
    return out


def read_apng(path):
    """-> (frames [n, H, W, 3] uint8, (delay_num, delay_den) of frame 0) of an APNG whose rows all carry filter type 0 and whose frames
    all cover the whole canvas; checks the signature, every chunk's CRC, the chunk order and the sequence numbers."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(raw):
        n, tag = struct.unpack(">I4s", raw[at:at + 8])
        data = raw[at + 8:at + 8 + n]
        assert struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        chunks.append((tag, data))
        at += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[1][0] == b"acTL" and chunks[-1][0] == b"IEND"
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    nframes, plays = struct.unpack(">II", chunks[1][1])
    frames, seq, delay = [], 0, None
    for tag, data in chunks[2:-1]:
        if tag == b"fcTL":
            s, w, h, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", data)
            assert (s, w, h, x, y, dispose, blend) == (seq, W, H, 0, 0, 0, 0)
            delay = delay or (num, den)
            seq += 1
            continue
        if tag == b"fdAT":
            assert struct.unpack(">I", data[:4])[0] == seq
            seq, data = seq + 1, data[4:]
        else:
            assert tag == b"IDAT" and not frames
        rows = np.frombuffer(zlib.decompress(data), dtype=np.uint8).reshape(H, 1 + 3 * W)
        assert (rows[:, 0] == 0).all()
        frames.append(rows[:, 1:].reshape(H, W, 3))
    assert len(frames) == nframes
    return np.stack(frames), delay


RASTER_P = (0, 1, 64, 257, 1024)
RASTER_CONFIGS = ((3, 36, 20), (1, 64, 64))                        # (I, W, H): edge tiles partial both ways; a viewport of a wider frame


def raster_tables(I, P, W, H, seed):
    """Random tables [I, P, 12] float32 for the raster tests: discs and capsules, radii 0, 0.5 and 3, alphas 1 and 0.35, ends up to
    8 px outside the image; record 0 a translucent capsule that spans every tile; from P >= 64 on, records 1..9 of every image are two
    capsules with ends hundreds of pixels outside, a NaN coordinate, an Inf radius, an Inf colour, alpha = 0, alpha < 0, r < 0 and a
    -Inf end."""
    rng = np.random.default_rng(seed)
    t = np.zeros((I, P, 12), dtype=np.float32)
    if P == 0:
        return t
    a = rng.uniform([-8, -8], [W + 8, H + 8], (I, P, 2))
    b = np.where(rng.random((I, P, 1)) < 0.4, a, a + rng.normal(0, 12, (I, P, 2)))
    t[:, :, 0:2], t[:, :, 2:4] = a, b
    t[:, :, 4] = rng.choice([0.0, 0.5, 3.0], (I, P))
    t[:, :, 5] = rng.choice([1.0, 0.35], (I, P))
    t[:, :, 6:9] = rng.uniform(0, 255, (I, P, 3))
    t[:, 0, :6] = [-5.0, -3.0, W + 5.0, H + 4.0, 3.0, 0.35]
    if P >= 64:
        t[:, 1, :4] = [-300.0, 10.0, W + 400.0, H - 5.0]
        t[:, 2, :4] = [W / 2.0, -250.0, W / 3.0, H + 500.0]
        t[:, 3, 0] = np.nan
        t[:, 4, 4] = np.inf
        t[:, 5, 7] = np.inf
        t[:, 6, 5] = 0.0
        t[:, 7, 5] = -1.0
        t[:, 8, 4] = -0.5
        t[:, 9, 3] = -np.inf
    return t


def raster_cases():
    """(I, W, H, P, tables) of every raster case."""
    return [(I, W, H, P, raster_tables(I, P, W, H, 100 * W + P)) for I, W, H in RASTER_CONFIGS for P in RASTER_P]


def scene_case(seed=5, F=5, N=7):
    """Host arrays of the scene test: F = 5 frames around (0.8, 0, 0.2) with a tilted floor; frame 1 has seg < 0, frame 2 a plane of
    zero normal, frame 3 two padding rows in its cloud, frame 4 its hips on the vertical (t16 - t12 along the plane's normal)."""
    rng = np.random.default_rng(seed)
    tgt = (rng.normal(0, 0.4, (F, 21, 3)) + np.array([0.8, 0.0, 0.2])).astype(np.float32)
    pred = (tgt + rng.normal(0, 0.06, (F, 21, 3))).astype(np.float32)
    ground = np.tile(np.array([0.1, -0.2, -1.0, 1.0], dtype=np.float32), (F, 1)) * rng.uniform(0.5, 2.0, (F, 1)).astype(np.float32)
    ground[2, :3] = 0.0
    cloud = np.concatenate([rng.normal([0.8, 0.0, 0.2], 0.4, (F, N, 3)), rng.uniform(1, 3, (F, N, 1)), rng.normal(0, 0.7, (F, N, 1)),
                            rng.uniform(10, 46, (F, N, 1))], axis=2).astype(np.float32)
    cloud[3, [2, 6]] = 0.0
    seg = np.array([0, -1, 0, 1, 1], dtype=np.int32)
    n = ground[4, :3].astype(np.float64)
    tgt[4, 16] = (tgt[4, 12].astype(np.float64) + 0.3 * n / np.linalg.norm(n)).astype(np.float32)
    return dict(pred=pred.reshape(F, 63), tgt=tgt.reshape(F, 63), ground=ground, cloud=cloud, seg=seg)
