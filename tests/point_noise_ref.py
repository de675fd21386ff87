"""numpy restatement of mmego_pack_frames_noise (the recipe in include/mmego_hip.h): frame_pack_ref's keep and place, and the noise of
every kept return in uint32 / float32 arithmetic, bit for bit.  A helper for tests/test_point_noise_cpu.py and
tests/test_point_noise_gpu.py."""
import numpy as np

import frame_pack_ref as ref

SALT_NOISE = 0x4E4F4953
SCALE = np.float32(float.fromhex("0x1.bb67aep-22"))          # fp32 nearest to sqrt(3) 2^-22
assert SCALE.view(np.uint32) == 0x34DDB3D7


def noise_z(n, q, seed):
    """z [n, 4] fp32 of the returns j = 0 .. n-1 of output frame q: columns x, y, z, velocity."""
    b = ref.keys(ref.dropout_key(seed, SALT_NOISE), q, np.arange(n)).astype(np.uint64)
    s = np.zeros((n, 4), dtype=np.int64)
    for c in range(4):
        for i in range(4):
            s[:, c] += ref.hash32((b + np.uint64(4 * c + i + 1)) & ref.M32) >> np.uint32(10)
    assert s.max(initial=0) < 1 << 24                         # (the conversion below is exact)
    return (s - 8388606).astype(np.float32) * SCALE


def perturb(raw, q, seed, sigma_xyz, sigma_v):
    """The raw points [n, 5] (x, y, z, intensity, velocity) of output frame q with their noise added: one rounded fp32 product and one
    rounded fp32 sum per channel; a channel whose sigma is 0 is copied."""
    raw = np.array(raw, dtype=np.float32).reshape(-1, 5)
    z = noise_z(len(raw), q, seed)
    if sigma_xyz != 0:
        raw[:, 0:3] = raw[:, 0:3] + np.float32(sigma_xyz) * z[:, 0:3]
    if sigma_v != 0:
        raw[:, 4] = raw[:, 4] + np.float32(sigma_v) * z[:, 3]
    return raw


def pack_frames_noise(pts, frame_off, frame_idx, pc_no, max_n, keep_p, seed, sigma_xyz, sigma_v):
    """The whole launch: -> out [nout, pc_no, 6] (r: the float64 norm of the perturbed x, y, z rounded to fp32, as frame_pack_ref.convert
    forms it), who [nout, pc_no] (the return in every slot; -1: a zero row)."""
    outs, whos = [], []
    for q, f in enumerate(np.asarray(frame_idx)):
        raw = np.asarray(pts[int(frame_off[f]):int(frame_off[f + 1])], dtype=np.float32).reshape(-1, 5)[:max_n]
        o, w = ref.pack_frame(perturb(raw, q, seed, sigma_xyz, sigma_v), q, pc_no, max_n, keep_p, seed)
        outs.append(o)
        whos.append(w)
    return np.stack(outs), np.stack(whos)
