"""Pictures of dense inference (`main.py --infer --dense --render DIR`, `--infer --vis`): the camera of a frame (host, float64), the two
device launches per view that turn frames into images (ops.render_prims builds every frame's table of 2-D primitives, ops.render_raster
composites it; csrc/render.hip, the recipe in include/mmego_hip.h), and an animated-PNG writer on zlib and struct alone."""
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops

VIEWS = ("front", "side")
CHUNK = 256                  # frames per launch pair: 256 x 1024 records of 48 bytes keep the primitive table under 13 MB
APNG_WORKERS = 8             # zlib releases the GIL; a fixed, small pool (never sized by the machine's CPU count)


def _unit(v, fallback=None):
    """Rows of v [F, 3] normalised; a row shorter than 1e-6 takes ``fallback``'s row (or stays 0).  -> (rows, which were long enough)."""
    n = np.linalg.norm(v, axis=1)
    ok = n > 1e-6
    out = np.where(ok[:, None], v / np.where(ok, n, 1.0)[:, None], 0.0 if fallback is None else fallback)
    return out, ok


def ring_axis(u):
    """e1 of the floor ring for unit normals u [F, 3] (float64): the coordinate axis with the smallest |u_i| (the first on ties) minus
    its component along u, normalised (render_math.h rd_ring_axes)."""
    e = np.eye(3)[np.argmin(np.abs(u), axis=1)]
    w = e - (e * u).sum(axis=1, keepdims=True) * u
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def camera(target, ground, view, size, metres=2.4):
    """cam [F, 8] float32, the 2 x 4 affine of every frame that ops.render_prims projects with: x_px = cam[0:3] . p + cam[3], y_px =
    cam[4:7] . p + cam[7].  target [F, 21, 3] (or [F, 63]) the RECORDED joints, ground [F, 4] the floor planes, both host arrays; computed
    in float64.  Up is the plane's unit normal u; where the plane has none (|n| <= 1e-6), the normalised t20 - t0.  The body's
    left-right axis l is t16 - t12 minus its component along up, normalised; where that is shorter than 1e-6, the ring's e1 of up.
    view "front": right = l; "side": right = up x l; up is up in both.  The scale is size / metres pixels per metre, target joint 0 lands
    on the image centre (size / 2, size / 2), and y grows downwards.  The camera follows the recorded skeleton, never the prediction,
    so an error is not hidden by the view.  The view is BODY-FIXED: the radar's frame moves with the head and no fixed world frame is
    available (on why there is no foot-sliding figure), so the picture shows pose, not travel."""
    if view not in VIEWS:
        raise ValueError("camera: view %r is not one of %s" % (view, ", ".join(VIEWS)))
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 1 or not (np.isfinite(metres) and metres > 0):
        raise ValueError("camera: size is a number of pixels >= 1 and metres a finite extent > 0, got %r and %r" % (size, metres))
    t = np.asarray(target, dtype=np.float64).reshape(-1, 21, 3)
    g = np.asarray(ground, dtype=np.float64).reshape(-1, 4)
    if len(g) != len(t):
        raise ValueError("camera: %d planes for %d frames" % (len(g), len(t)))
    spine, _ = _unit(t[:, 20] - t[:, 0], np.array([0.0, 0.0, 1.0]))
    up, _ = _unit(g[:, :3], spine)
    hips = t[:, 16] - t[:, 12]
    left, _ = _unit(hips - (hips * up).sum(axis=1, keepdims=True) * up, ring_axis(up))
    right = left if view == "front" else np.cross(up, left)
    s, c = float(size) / float(metres), float(size) / 2.0
    cam = np.empty((len(t), 8), dtype=np.float64)
    cam[:, 0:3], cam[:, 4:7] = s * right, -s * up
    cam[:, 3] = c - s * (right * t[:, 0]).sum(axis=1)
    cam[:, 7] = c + s * (up * t[:, 0]).sum(axis=1)
    return cam.astype(np.float32)


def render_frames(pred, tgt, ground, cloud, seg, size, vmax=1.0):
    """Device uint8 [F, size, 2 size, 3]: every frame's front view in the left half and its side view in the right half, two
    ops.render_prims + ops.render_raster pairs through the row pitch, in chunks of at most CHUNK frames.  pred, tgt [F, >= 63], ground
    [F, 4], cloud [F, N, 6] device tensors, seg [F] int32 (< 0: the target alone).  The cameras come from camera(): one small
    device -> host read of tgt and ground, one upload per view."""
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 16 <= size <= 1024 or size % 4:
        raise ValueError("render_frames: size is a multiple of 4 in [16, 1024], got %r" % (size,))
    F, dev, size = pred.shape[0], pred.device, int(size)
    seg = ops._seg_on(seg, F, dev, "render_frames")
    tgt_h, ground_h = tgt[:, :63].cpu().numpy(), ground.cpu().numpy()
    cams = [torch.as_tensor(camera(tgt_h, ground_h, v, size)).to(dev) for v in VIEWS]
    out = torch.empty((F, size, 2 * size, 3), dtype=torch.uint8, device=dev)
    prims = torch.empty((min(F, CHUNK), ops.RENDER_FIXED + cloud.shape[1], ops.RENDER_REC), dtype=torch.float32, device=dev)
    for a in range(0, F, CHUNK):
        e = min(a + CHUNK, F)
        for v, cam in enumerate(cams):
            ops.render_prims(pred[a:e], tgt[a:e], ground[a:e], cloud[a:e], seg[a:e], cam[a:e], vmax, prims[:e - a])
            ops.render_raster(prims[:e - a], out[a:e, :, v * size:(v + 1) * size])
    return out


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_apng(path, frames, fps):
    """An animated PNG of frames [n, H, W, 3] (uint8, host) at ``fps`` frames per second, played for ever; the first frame is the still
    image a viewer without APNG support shows.  Chunks: IHDR, acTL, then per frame fcTL with IDAT (frame 0) or fdAT, then IEND; 8-bit
    RGB, filter type 0 on every row, zlib level 6, compressed on a pool of at most APNG_WORKERS threads.  Needs zlib and struct only."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or 0 in frames.shape:
        raise ValueError("write_apng: frames is uint8 [n >= 1, H, W, 3], got %s %s" % (frames.dtype, frames.shape))
    if isinstance(fps, bool) or not isinstance(fps, (int, np.integer)) or not 1 <= fps <= 100:
        raise ValueError("write_apng: fps is an integer in [1, 100], got %r" % (fps,))
    n, H, W = frames.shape[:3]

    def packed(i):                                                 # every row behind its filter byte 0
        raw = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
        raw[:, 1:] = frames[i].reshape(H, 3 * W)
        return zlib.compress(raw.tobytes(), 6)

    with ThreadPoolExecutor(max_workers=min(APNG_WORKERS, n)) as pool:
        data = list(pool.map(packed, range(n)))
    parts = [b"\x89PNG\r\n\x1a\n", _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)), _chunk(b"acTL", struct.pack(">II", n, 0))]
    seq = 0
    for i, z in enumerate(data):
        parts.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, 1, int(fps), 0, 0)))
        seq += 1
        if i == 0:
            parts.append(_chunk(b"IDAT", z))
        else:
            parts.append(_chunk(b"fdAT", struct.pack(">I", seq) + z))
            seq += 1
    parts.append(_chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(b"".join(parts))
    return path
