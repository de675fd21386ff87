"""What dense inference's blend in rotation space (dense.dense_infer(blend_space="rot"): --infer --dense --blend_space rot) costs
beside the bone-direction blend, in ONE process:

  python scripts/bench_dense_rot.py OUT.json

(a) device-event time of the two blend launches of a pass in either form, on the same plan and the same window rows, at the largest
    shape of the real layout (tests/golden/g11_loader.npz, stride 1: 19 114 frames, 14 877 windows, cover up to 20; the plan
    scripts/bench_dense_bones.py timed): mmego_blend_rot on the upper rows (J = 15, NQ = 14, with both spreads and the fallback counts)
    and the lower rows (J = 8, NQ = 6), beside mmego_blend_bones on the same rows -- the forms alternating, 20 chains of 10 pairs after
    3, a chain per event pair so that the timed window is not a single launch.  The rotations are random proper ones, the same per bone
    within 0.5 rad over the rows, so that no bone takes the fallback;
(b) the dense pass, wall clock to its last host read, on Sample_data-shaped synthetic frames (scripts/bench_frame_store.py's generator:
    223 recordings, about 19 100 frames; frame_no 20, window minibatch 64) at strides 5 and 1 with blend_space="bones" and "rot" --
    alternating, five rounds, medians, and the band of the rounds; and the share of a "rot" pass that its two blend calls are, measured
    in place: device events around the two ops.blend_rot calls of one further pass per stride ("blend_rot x 2 inside a pass");
(c) what it reports on those frames with the committed pretrained weights: rot_spread_deg, bone_dev_cm, degenerate_bones, spread_cm and
    the five reference figures for either space.  Random clouds: no error figure says anything about accuracy."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_frame_store import rounds, synthetic_frames  # noqa: E402
from mmego_amd import dense, hip, nets, ops, processors, skeleton  # noqa: E402
from mmego_amd.config import ConfigDemo  # noqa: E402
from mmego_amd.data import DensePlan, PosePC  # noqa: E402

dev = torch.device("cuda:0")
T, B = 20, 64
CHAIN = 10


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


def load(module, npz):
    module.load_state_dict({k: torch.tensor(npz[k]) for k in npz.files})
    return module.to(dev).eval()


def chains_us(forms, reps=20, warm=3):
    """Per form: device-event time of CHAIN back-to-back calls, over CHAIN; the forms alternate inside every repetition."""
    for _ in range(warm):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CHAIN):
                f()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / CHAIN)
    return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()}


def rotations(rng, n, nq):
    """[n, nq, 9] float32: per rotation slot one random base rotation, per row a perturbation of at most 0.5 rad (host, float64)."""
    def rodrigues(axis, angle):
        axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
        K = np.zeros(axis.shape[:-1] + (3, 3))
        K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -axis[..., 2], axis[..., 1], axis[..., 2]
        K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -axis[..., 0], -axis[..., 1], axis[..., 0]
        s, c = np.sin(angle)[..., None, None], np.cos(angle)[..., None, None]
        return np.eye(3) + s * K + (1 - c) * (K @ K)
    base = rodrigues(rng.normal(size=(nq, 3)), rng.uniform(-np.pi, np.pi, nq))
    P = rodrigues(rng.normal(size=(n, nq, 3)), rng.uniform(-0.5, 0.5, (n, nq)))
    return (base[None] @ P).reshape(n, nq, 9).astype(np.float32)


def main(path):
    hip.lib()
    ConfigDemo.gt_head_pose = True
    base = processors._Base(ConfigDemo, make_dirs=False)
    up, lo = load(nets.UpperNet(), golden("w_upper_pretrained.npz")), load(nets.LowerNet(64), golden("w_lower_pretrained.npz"))
    res = {"shape": {"frame_no": T, "window_minibatch": B},
           "method": "launches: device events around a chain of %d calls, the forms alternating, 20 repetitions after 3, per call; passes: "
                     "wall clock around a whole pass (its last statement is a device -> host read), one warm pass each, then the passes "
                     "alternating, five rounds, medians" % CHAIN}

    # (a) the launches at the largest shape
    plan = DensePlan(golden("g11_loader.npz")["dec.snip_len"].astype(np.int64), T, 1)
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    n = plan.W * T
    src_up, src_lo = torch.randn((n, 45), device=dev, generator=g), torch.randn((n, 24), device=dev, generator=g)
    q_up, q_lo = torch.as_tensor(rotations(rng, n, 14)).to(dev), torch.as_tensor(rotations(rng, n, 6)).to(dev)
    Rh = torch.eye(3, device=dev).reshape(1, 9).repeat(n, 1).contiguous()
    up_f, lo_f = torch.empty((plan.F, 45), device=dev), torch.empty((plan.F, 24), device=dev)
    spread, rot_spread = torch.empty(plan.F, device=dev), torch.empty(plan.F, device=dev)
    quat_up, quat_lo = torch.empty((plan.F, 14, 4), device=dev), torch.empty((plan.F, 6, 4), device=dev)
    fell = torch.zeros((2, plan.F), dtype=torch.int32, device=dev)
    body = rng.normal(0, 0.2, (20, 3)).astype(np.float32)
    L = np.linalg.norm(body.astype(np.float64), axis=1).astype(np.float32)

    ops.blend_bones(src_up, plan, skeleton.WALK_UPPER, L[:14], up_f, spread, fell[0])      # (the host checks and uploads happen here, once)
    off, row, w = plan._cover_dev[str(dev)]
    (bu, lu, _), (bl, ll, _) = ops._bones_on(skeleton.WALK_UPPER, L[:14], 15, dev, "bench"), ops._bones_on(skeleton.WALK_LOWER, L[14:], 8, dev, "bench")
    ru, rl = (torch.as_tensor(np.asarray(r, dtype=np.int32)).to(dev) for r in (skeleton.ROT_UPPER, skeleton.ROT_LOWER))
    body_u, body_l = torch.as_tensor(body[:14].copy()).to(dev), torch.as_tensor(body[14:].copy()).to(dev)

    def bones():
        hip.call("blend_bones", src_up, n, 15, off, row, w, plan.F, bu, lu, 14, up_f, 45, spread, fell[0])
        hip.call("blend_bones", src_lo, n, 8, off, row, w, plan.F, bl, ll, 6, lo_f, 24, None, fell[1])

    def rot():
        hip.call("blend_rot", src_up, n, 15, q_up, 14, Rh, off, row, w, plan.F, bu, ru, body_u, 14, up_f, 45, quat_up, spread, rot_spread, fell[0])
        hip.call("blend_rot", src_lo, n, 8, q_lo, 6, Rh, off, row, w, plan.F, bl, rl, body_l, 6, lo_f, 24, quat_lo, None, None, fell[1])

    nnz = len(plan.cov_row)
    cover_bytes = 2 * (nnz * 8 + (plan.F + 1) * 8)
    bones_bytes = nnz * (45 + 24) * 4 + cover_bytes + plan.F * (45 + 24 + 1) * 4
    rot_bytes = nnz * (45 + 24 + 9 * (14 + 6) + 2 * 9) * 4 + cover_bytes + plan.F * (45 + 24 + 2 + 4 * 20) * 4
    us = chains_us({"blend_bones x 2 (J = 15 with spread, J = 8; fallback counts)": bones,
                    "blend_rot x 2 (J = 15 with both spreads, J = 8; quaternions, fallback counts)": rot})
    res["launch_us"] = {"F": plan.F, "windows": plan.W, "cover_entries": nnz, "max_cover": plan.max_cover,
                        "bytes_of_the_blend_bones_pair": bones_bytes, "bytes_of_the_blend_rot_pair": rot_bytes,
                        "eigen_solves_per_launch_pair": plan.F * 20}
    for (k, v), nbytes in zip(us.items(), (bones_bytes, rot_bytes)):
        res["launch_us"][k] = dict(v, tb_per_s=round(nbytes / v["median"] / 1e6, 3))
    a, b = (us[k]["median"] for k in us)
    res["launch_us"]["rot_over_bones"] = round(b / a, 3)
    res["launch_us"]["fallbacks"] = int(fell.sum())
    print("launch_us", res["launch_us"])

    # (b) the pass
    dec = synthetic_frames()
    PosePC._decode = lambda self: dec
    np.random.seed(0)
    ds = PosePC(train=False, vis=True, batch_length=T, root=os.path.join(ROOT, "scripts"), keep_frames=True)
    res["frames"] = int(len(ds.frame_npts_))

    def timed_pass(stride, **more):
        def s():
            t0 = time.perf_counter()
            dense.dense_infer(base, None, up, lo, ds, stride, batch_size=B, **more)
            return time.perf_counter() - t0
        return s
    timers = {}
    for stride in (5, 1):
        timers["stride %d, bones" % stride] = timed_pass(stride, blend_space="bones")
        timers["stride %d, rot" % stride] = timed_pass(stride, blend_space="rot")
    for t in timers.values():
        t()
    res["pass_s"] = rounds(timers, 5)
    # the two blend_rot launches where they run: device events around them inside one more pass per stride
    inside = {}
    real = ops.blend_rot

    def timed(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real(*a, **k)
        e1.record()
        inside.setdefault("events", []).append((e0, e1))
        return out
    for stride in (5, 1):
        bones_s, rot_s = (res["pass_s"]["stride %d, %s" % (stride, k)] for k in ("bones", "rot"))
        band = (max(bones_s["rounds"]) - min(bones_s["rounds"])) / bones_s["median"]
        res["pass_s"]["stride %d: band of the bones rounds / median" % stride] = round(band, 4)
        res["pass_s"]["stride %d: rot / bones" % stride] = round(rot_s["median"] / bones_s["median"], 4)
        inside.clear()
        ops.blend_rot = timed
        try:
            dense.dense_infer(base, None, up, lo, ds, stride, batch_size=B, blend_space="rot")
        finally:
            ops.blend_rot = real
        torch.cuda.synchronize()
        ms = sum(e0.elapsed_time(e1) for e0, e1 in inside["events"])
        res["pass_s"]["stride %d: blend_rot x 2 inside a pass, ms (host checks and uploads included)" % stride] = round(ms, 3)
        res["pass_s"]["stride %d: that over the rot pass" % stride] = round(ms / 1e3 / rot_s["median"], 4)
    print("pass_s", res["pass_s"])

    # (c) the figures
    res["figures_synthetic"] = {"note": "pretrained weights on random clouds: the error figures show the mechanics, not accuracy"}
    for stride in (10, 5, 1):
        for space in ("bones", "rot"):
            s, _ = dense.dense_infer(base, None, up, lo, ds, stride, batch_size=B, blend_space=space)
            keys = ("bone_dev_cm", "single_bone_dev_cm", "all_cm", "upper_cm", "lower_cm", "rot_deg", "spread_cm") + (("rot_spread_deg",) if space == "rot" else ())
            res["figures_synthetic"]["stride %d %s" % (stride, space)] = dict({k: round(float(s[k]), 5) for k in keys},
                                                                            degenerate_bones=s["degenerate_bones"])
    print("figures_synthetic", res["figures_synthetic"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "dense_rot.json")
