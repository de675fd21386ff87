"""numpy restatement of mmego_pack_frames (the recipe in include/mmego_hip.h), in uint32 arithmetic; the order of slots and of
survivors comes from a stable argsort of the keys.  A helper for tests/test_frame_store_cpu.py and tests/test_frame_pack_gpu.py."""
import numpy as np

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
SALT_KEEP, SALT_ORDER = 0x4B454550, 0x4F524452


def hash32(x):
    """csrc/common.h hash32 on a uint32 array (or scalar)."""
    x = np.asarray(x, dtype=np.uint64) & M32          # (uint64 words masked to 32 bits: no overflow warnings)
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x.astype(np.uint32)


def dropout_key(seed, salt):
    """csrc/common.h dropout_key: a 64-bit LCG step of (seed, salt), folded to 32 bits and hashed."""
    s = ((int(seed) & M64) + salt * 0x9E3779B97F4A7C15) & M64
    s = (s * 6364136223846793005 + 1442695040888963407) & M64
    return int(hash32(((s & M32) + 0x9E3779B9 * (s >> 32)) & M32))


def keys(K, q, i):
    """key(K, q, i) = hash32(hash32(K ^ hash32(q)) ^ i) for an array of i."""
    fk = int(hash32(K ^ int(hash32(q & M32))))
    return hash32(np.asarray(i, dtype=np.uint64) ^ fk)


def convert(raw):
    """(n, 5) x, y, z, intensity, velocity -> (n, 6) x, y, z, r, velocity, intensity as data.pack_points computes it (r: float64 norm
    rounded to fp32)."""
    raw = np.asarray(raw, dtype=np.float32)
    out = np.zeros((len(raw), 6), dtype=np.float32)
    out[:, 0:3] = raw[:, :3]
    out[:, 3] = np.linalg.norm(raw[:, 0:3].astype(np.float64), axis=1)
    out[:, 4] = raw[:, 4]
    out[:, 5] = raw[:, 3]
    return out


def kept_points(n, q, keep_p, seed):
    """The numbers of the points of an n-point frame that survive as output frame q, increasing."""
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    j = np.arange(n)
    u = (keys(dropout_key(seed, SALT_KEEP), q, j) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    kept = j[u < np.float32(keep_p)]
    if len(kept) == 0:
        ko = keys(dropout_key(seed, SALT_ORDER), q, j)
        kept = j[np.argsort(ko, kind="stable")[:1]]
    return kept


def pack_frame(raw, q, pc_no, max_n, keep_p, seed):
    """One output frame [pc_no, 6] from the raw points [n, 5] of its frame; also the point number in every slot (-1: a zero row)."""
    raw = np.asarray(raw, dtype=np.float32).reshape(-1, 5)[:max_n]
    n = len(raw)
    pts = convert(raw)
    kept = kept_points(n, q, keep_p, seed)
    KO = dropout_key(seed, SALT_ORDER)
    out, who = np.zeros((pc_no, 6), dtype=np.float32), np.full(pc_no, -1, dtype=np.int64)
    if len(kept) < pc_no:
        order = np.argsort(keys(KO, q, np.arange(pc_no)), kind="stable")      # order[r]: the slot of rank r
        who[order[:len(kept)]] = kept
    else:
        order = np.argsort(keys(KO, q, kept), kind="stable")                  # order[r]: the survivor of rank r
        who[:] = kept[order[:pc_no]]
    out[who >= 0] = pts[who[who >= 0]]
    return out, who


def pack_frames(pts, frame_off, frame_idx, pc_no, max_n, keep_p, seed):
    """The whole launch: -> out [nout, pc_no, 6], who [nout, pc_no]."""
    outs, whos = [], []
    for q, f in enumerate(np.asarray(frame_idx)):
        o, w = pack_frame(pts[int(frame_off[f]):int(frame_off[f + 1])], q, pc_no, max_n, keep_p, seed)
        outs.append(o)
        whos.append(w)
    return np.stack(outs), np.stack(whos)
