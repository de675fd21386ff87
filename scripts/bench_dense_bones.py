"""What the bone-length-preserving blend of dense inference (dense.dense_infer(blend_space="bones"): --infer --dense --blend_space
bones) costs and changes, in ONE process:

  python scripts/bench_dense_bones.py OUT.json

(a) device-event time of the two blend launches of a pass in either form, at the largest shape of the real layout
    (tests/golden/g11_loader.npz, stride 1: 19 114 frames, 14 877 windows, cover up to 20; the plan scripts/bench_dense_infer.py timed):
    mmego_blend_bones on the upper rows (J = 15, with spread and the fallback counts) and the lower rows (J = 8), beside
    mmego_blend_windows at C = 45 with spread and at C = 24 -- the forms alternating, 20 chains of 10 pairs after 3, a chain per event pair
    so that the timed window is not a single launch; the four mmego_bone_length_dev launches and their two column sums as well;
(b) the dense pass, wall clock to its last host read, on Sample_data-shaped synthetic frames (scripts/bench_frame_store.py's generator:
    223 recordings, about 19 100 frames; frame_no 20, window minibatch 64) at strides 5 and 1: without the argument (the launches of the
    pass before this option, bit for bit), blend_space="joints" (those launches plus the bone-length figures) and "bones" -- alternating,
    five rounds, medians, and the band of the rounds;
(c) what it changes, with the committed pretrained weights on the synthetic frames, --metrics full, both blends, strides 10, 5 and 1:
    bone deviation, the five reference figures and the stitched acceleration error for either space.  Random clouds: the nets' windows
    disagree far more than on real data and no error figure says anything about accuracy; only the deviation figure carries meaning."""
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
    n = plan.W * T
    src_up, src_lo = torch.randn((n, 45), device=dev, generator=g), torch.randn((n, 24), device=dev, generator=g)
    up_f, lo_f, spread = torch.empty((plan.F, 45), device=dev), torch.empty((plan.F, 24), device=dev), torch.empty(plan.F, device=dev)
    fell = torch.zeros((2, plan.F), dtype=torch.int32, device=dev)
    L_up, L_lo = np.full(14, 0.25, np.float32), np.full(6, 0.4, np.float32)
    D, Dw, sums = torch.empty((plan.F, 20), device=dev), torch.empty((n, 20), device=dev), torch.zeros((2, 20), device=dev)

    ops.blend_bones(src_up, plan, skeleton.WALK_UPPER, L_up, up_f, spread, fell[0])      # (the host checks and uploads happen here, once)
    off, row, w = plan._cover_dev[str(dev)]
    (bu, lu, _), (bl, ll, _) = ops._bones_on(skeleton.WALK_UPPER, L_up, 15, dev, "bench"), ops._bones_on(skeleton.WALK_LOWER, L_lo, 8, dev, "bench")
    Dl, Dwl = D[:, 14:], Dw[:, 14:]

    def joints():
        hip.call("blend_windows", src_up, n, 45, off, row, w, plan.F, up_f, 45, spread)
        hip.call("blend_windows", src_lo, n, 24, off, row, w, plan.F, lo_f, 24, None)

    def bones():
        hip.call("blend_bones", src_up, n, 15, off, row, w, plan.F, bu, lu, 14, up_f, 45, spread, fell[0])
        hip.call("blend_bones", src_lo, n, 8, off, row, w, plan.F, bl, ll, 6, lo_f, 24, None, fell[1])

    def figures():
        hip.call("bone_length_dev", up_f, 45, plan.F, 15, bu, lu, 14, D, 20)
        hip.call("bone_length_dev", lo_f, 24, plan.F, 8, bl, ll, 6, Dl, 20)
        hip.call("bone_length_dev", src_up, 45, n, 15, bu, lu, 14, Dw, 20)
        hip.call("bone_length_dev", src_lo, 24, n, 8, bl, ll, 6, Dwl, 20)
        ops.colsum(D, sums[0])
        ops.colsum(Dw, sums[1])

    nnz = len(plan.cov_row)
    blend_bytes = nnz * (45 + 24) * 4 + 2 * (nnz * 8 + (plan.F + 1) * 8) + plan.F * (45 + 24 + 1) * 4
    us = chains_us({"blend_windows x 2 (C = 45 with spread, C = 24)": joints, "blend_bones x 2 (J = 15 with spread, J = 8; fallback counts)": bones,
                    "bone_length_dev x 4 + colsum x 2": figures})
    res["launch_us"] = {"F": plan.F, "windows": plan.W, "cover_entries": nnz, "max_cover": plan.max_cover, "bytes_of_either_blend_pair": blend_bytes}
    for k, v in us.items():
        res["launch_us"][k] = dict(v, tb_per_s=round(blend_bytes / v["median"] / 1e6, 3)) if k.startswith("blend") else v
    a, b = (us[k]["median"] for k in list(us)[:2])
    res["launch_us"]["bones_over_joints"] = round(b / a, 3)
    assert int(fell.sum()) == 0
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
        timers["stride %d, no argument" % stride] = timed_pass(stride)
        timers["stride %d, joints" % stride] = timed_pass(stride, blend_space="joints")
        timers["stride %d, bones" % stride] = timed_pass(stride, blend_space="bones")
    for t in timers.values():
        t()
    res["pass_s"] = rounds(timers, 5)
    for stride in (5, 1):
        base_s = res["pass_s"]["stride %d, no argument" % stride]
        band = (max(base_s["rounds"]) - min(base_s["rounds"])) / base_s["median"]
        res["pass_s"]["stride %d: band of the no-argument rounds / median" % stride] = round(band, 4)
        for k in ("joints", "bones"):
            res["pass_s"]["stride %d: %s / no argument" % (stride, k)] = round(res["pass_s"]["stride %d, %s" % (stride, k)]["median"] / base_s["median"], 4)
    print("pass_s", res["pass_s"])

    # (c) the effect
    res["effect_synthetic"] = {"note": "pretrained weights on random clouds: only bone_dev_cm carries meaning; the error figures show the "
                                       "mechanics, not accuracy"}
    for blend in ("mean", "triangle"):
        for stride in (10, 5, 1):
            for space in ("joints", "bones"):
                s, _ = dense.dense_infer(base, None, up, lo, ds, stride, blend=blend, batch_size=B, metrics="full", blend_space=space)
                res["effect_synthetic"]["%s stride %d %s" % (blend, stride, space)] = {
                    k: round(float(s[k]), 5) for k in ("bone_dev_cm", "single_bone_dev_cm", "all_cm", "upper_cm", "lower_cm", "rot_deg",
                                                       "spread_cm", "accel_cm", "root_rel_cm", "pa_cm")}
                res["effect_synthetic"]["%s stride %d %s" % (blend, stride, space)].update(
                    degenerate_bones=s["degenerate_bones"], per_joint_cm=[round(float(v), 3) for v in s["per_joint_cm"]])
    print("effect_synthetic", res["effect_synthetic"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "dense_bones.json")
