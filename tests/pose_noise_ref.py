"""numpy restatement of mmego_pose_jitter (the recipe in include/mmego_hip.h): hash32 and dropout_key in uint32 / uint64 arithmetic, the
six draws of a row as exact integers times the fp32 scale, and the perturbation in float64.  A helper for tests/test_pose_noise_*.py."""
import numpy as np

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
SALT = 0x504F5345
SCALE = np.float32(float.fromhex("0x1.bb67aep-22"))          # fp32 nearest to sqrt(3) 2^-22
assert SCALE.view(np.uint32) == 0x34DDB3D7


def hash32(x):
    """csrc/common.h hash32 on a uint32 array (or scalar)."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M32
    x = x ^ (x >> 16)
    return x.astype(np.uint32)


def dropout_key(seed, salt):
    """csrc/common.h dropout_key: a 64-bit LCG step of (seed, salt), folded to 32 bits and hashed."""
    s = ((int(seed) & M64) + salt * 0x9E3779B97F4A7C15) & M64
    s = (s * 6364136223846793005 + 1442695040888963407) & M64
    return int(hash32(((s & M32) + 0x9E3779B9 * (s >> 32)) & M32))


def draws(word, d):
    """z [len(d), 6] fp32 of the rows whose draw numbers are d (int64; the kernel takes their low 32 bits) under the seed word."""
    d = np.asarray(d, dtype=np.int64).astype(np.uint64) & M32
    K = dropout_key(word, SALT)
    b = hash32(hash32(d).astype(np.uint64) ^ np.uint64(K)).astype(np.uint64)
    s = np.zeros((len(d), 6), dtype=np.int64)
    for c in range(6):
        for i in range(4):
            s[:, c] += hash32((b + np.uint64(4 * c + i + 1)) & M32) >> np.uint32(10)
    assert s.max(initial=0) < 1 << 24                         # (the conversion below is exact)
    return (s - 8388606).astype(np.float32) * SCALE


def rotations(sigma_deg, z):
    """E [n, 3, 3] float64 of the rotation vectors (sigma_deg pi / 180) z[:, :3]: Rodrigues, the series below theta = 1e-3."""
    w = (float(sigma_deg) * (np.pi / 180.0)) * z[:, :3].astype(np.float64)
    q = (w * w).sum(axis=1)
    th = np.sqrt(q)
    small = th < 1e-3
    safe = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - q / 6.0 + q * q / 120.0, np.sin(safe) / safe)
    b = np.where(small, 0.5 - q / 24.0 + q * q / 720.0, (1.0 - np.cos(safe)) / (safe * safe))
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    return np.eye(3)[None] + a[:, None, None] * K + b[:, None, None] * (K @ K)


def pose_jitter(R, t, sigma_deg, sigma_t, word, ids=None):
    """-> (R' [n, 3, 3], t' [n, 3]) in float64, before the one float rounding of the kernel's store; a sigma of 0 returns its input."""
    R = np.asarray(R, dtype=np.float32).reshape(-1, 3, 3)
    t = np.asarray(t, dtype=np.float32).reshape(-1, 3)
    z = draws(word, np.arange(len(R)) if ids is None else ids)
    Rn = rotations(sigma_deg, z) @ R.astype(np.float64) if sigma_deg != 0 else R.astype(np.float64)
    tn = t.astype(np.float64) + float(sigma_t) * z[:, 3:].astype(np.float64) if sigma_t != 0 else t.astype(np.float64)
    return Rn, tn


def rotation_vectors(E):
    """The rotation vectors [n, 3] of rotations E [n, 3, 3] (float64; angles well below pi): the axis from the skew part."""
    v = 0.5 * np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], axis=1)      # sin(theta) axis
    s = np.linalg.norm(v, axis=1)
    th = np.arctan2(s, 0.5 * (np.trace(E, axis1=1, axis2=2) - 1.0))
    return v * np.where(s > 1e-12, th / np.where(s > 1e-12, s, 1.0), 1.0)[:, None]
