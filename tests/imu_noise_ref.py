"""numpy restatement of mmego_imu_jitter (the recipe in include/mmego_hip.h): the nine draws of a sample and the nine of its window as
exact integers times the fp32 scale, and the perturbation in float64 before the one float rounding of the kernel's store.  hash32,
dropout_key and Rodrigues are tests/pose_noise_ref.py's.  A helper for tests/test_imu_noise_*.py."""
import numpy as np

from pose_noise_ref import M32, SCALE, dropout_key, hash32, rotations

SALT_SAMPLE, SALT_WINDOW = 0x494D554E, 0x494D5542


def draws(word, salt, numbers):
    """z [len(numbers), 9] fp32 of the draw numbers (any integers: the kernel takes their low 32 bits) under the seed word and the salt."""
    e = np.asarray(numbers, dtype=np.int64).astype(np.uint64) & M32
    K = dropout_key(word, salt)
    b = hash32(hash32(e).astype(np.uint64) ^ np.uint64(K)).astype(np.uint64)
    s = np.zeros((len(e), 9), dtype=np.int64)
    for c in range(9):
        for i in range(4):
            s[:, c] += hash32((b + np.uint64(4 * c + i + 1)) & M32) >> np.uint32(10)
    assert s.max(initial=0) < 1 << 24                         # (the conversion below is exact)
    return (s - 8388606).astype(np.float32) * SCALE


def sample_draws(word, n_rows, S, row_ids=None):
    """z_s [n_rows S, 9]: sample s of row i has draw number d S + s, d = row_ids[i] or i."""
    d = np.arange(n_rows, dtype=np.int64) if row_ids is None else np.asarray(row_ids, dtype=np.int64)
    with np.errstate(over="ignore"):
        e = (d[:, None] * np.int64(S) + np.arange(S, dtype=np.int64)[None]).reshape(-1)
    return draws(word, SALT_SAMPLE, e)


def window_draws(word, n_rows, T, S, win_ids=None):
    """z_w [n_rows S, 9]: every sample of every row of window i / T sees the draws of u = win_ids[i / T] or i / T."""
    u = np.arange(n_rows // T, dtype=np.int64) if win_ids is None else np.asarray(win_ids, dtype=np.int64)
    return np.repeat(draws(word, SALT_WINDOW, u), T * S, axis=0)


def imu_jitter(imu, T, sigmas, word, row_ids=None, win_ids=None):
    """-> imu' [n_rows, S, 15] in float64; a group both of whose sigmas are 0 returns its input."""
    imu = np.asarray(imu, dtype=np.float32)
    S = imu.shape[-2]
    x = imu.reshape(-1, 15).astype(np.float64)
    n_rows = len(x) // S
    assert n_rows % T == 0
    n_rot, n_acc, n_gyro, b_rot, b_acc, b_gyro = (float(v) for v in sigmas)
    zs = sample_draws(word, n_rows, S, row_ids)
    zw = window_draws(word, n_rows, T, S, win_ids)
    out = x.copy()
    if n_rot != 0 or b_rot != 0:
        if b_rot == 0:
            E = rotations(n_rot, zs)
        elif n_rot == 0:
            E = rotations(b_rot, zw)
        else:
            E = rotations(n_rot, zs) @ rotations(b_rot, zw)
        out[:, :9] = (E @ x[:, :9].reshape(-1, 3, 3)).reshape(-1, 9)
    for lo, noise, bias in ((9, n_acc, b_acc), (12, n_gyro, b_gyro)):
        if noise != 0 or bias != 0:
            c = lo - 6                                        # the group's draw channels: 3 .. 5, 6 .. 8
            out[:, lo:lo + 3] = (x[:, lo:lo + 3] + bias * zw[:, c:c + 3].astype(np.float64)) + noise * zs[:, c:c + 3].astype(np.float64)
    return out.reshape(n_rows, S, 15)
