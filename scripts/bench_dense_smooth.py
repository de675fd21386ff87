"""What the temporal filter of dense inference (dense.dense_infer(smooth=(H, order, taper)): --infer --dense --smooth H) costs and
changes, in ONE process:

  python scripts/bench_dense_smooth.py OUT.json

(a) device-event time of the filter's launches alone at the frame count of the real layout (tests/golden/g11_loader.npz: 19 114 frames in
    223 recordings, every frame of a recording of at least frame_no frames its recording's segment): mmego_smooth_frames and
    mmego_smooth_bones at C = 45 (with moved; the bones form with its fallback counts) and C = 24, order 2, the gauss taper, H = 2, 8 and
    31; beside them, as the yardstick, the mmego_blend_windows launches of the stride-1 plan at the same F (C = 45 with spread, C = 24)
    -- the forms alternating, 20 chains of 10 calls after 3, a chain per event pair so that the timed window is not a single launch;
(b) the dense pass, wall clock to its last host read, on Sample_data-shaped synthetic frames (scripts/bench_frame_store.py's generator:
    223 recordings, about 19 100 frames; frame_no 20, window minibatch 64) at strides 5 and 1: without the argument (the launches of the
    pass before this option) and with smooth=(8, 2, "gauss"), in either blend space -- alternating, five rounds, medians, and the band
    of the rounds;
(c) what it changes, with the committed pretrained weights on the synthetic frames, --metrics full, stride 5: the displacement, the
    acceleration error before and after, the joint error before and after, the bone deviation in either space, for H = 2, 8, 31 and the
    three orders.  Random clouds and random targets: the windows disagree far more than on real data, and no error figure says anything
    about accuracy; the acceleration figures show the mechanics only."""
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
from bench_dense_bones import chains_us, golden, load  # noqa: E402
from bench_frame_store import rounds, synthetic_frames  # noqa: E402
from mmego_amd import dense, hip, nets, ops, processors, skeleton  # noqa: E402
from mmego_amd.config import ConfigDemo  # noqa: E402
from mmego_amd.data import DensePlan, PosePC  # noqa: E402

dev = torch.device("cuda:0")
T, B = 20, 64
HS = (2, 8, 31)


def main(path):
    hip.lib()
    ConfigDemo.gt_head_pose = True
    base = processors._Base(ConfigDemo, make_dirs=False)
    up, lo = load(nets.UpperNet(), golden("w_upper_pretrained.npz")), load(nets.LowerNet(64), golden("w_lower_pretrained.npz"))
    res = {"shape": {"frame_no": T, "window_minibatch": B},
           "method": "launches: device events around a chain of 10 calls, the forms alternating, 20 repetitions after 3, per call; passes: "
                     "wall clock around a whole pass (its last statement is a device -> host read), one warm pass each, then the passes "
                     "alternating, five rounds, medians"}

    # (a) the launches
    plan = DensePlan(golden("g11_loader.npz")["dec.snip_len"].astype(np.int64), T, 1)
    F, n = plan.F, plan.W * T
    g = torch.Generator(device=dev).manual_seed(0)
    win_up, win_lo = torch.randn((n, 45), device=dev, generator=g), torch.randn((n, 24), device=dev, generator=g)
    src = {45: torch.randn((F, 45), device=dev, generator=g), 24: torch.randn((F, 24), device=dev, generator=g)}
    dst = {45: torch.empty((F, 45), device=dev), 24: torch.empty((F, 24), device=dev)}
    moved, spread = torch.empty(F, device=dev), torch.empty(F, device=dev)
    fell = torch.zeros(F, dtype=torch.int32, device=dev)
    seg = torch.as_tensor(np.where(plan.covered != 0, plan.frame_rec, -1).astype(np.int32)).to(dev)
    L_up, L_lo = np.full(14, 0.25, np.float32), np.full(6, 0.4, np.float32)
    (bu, lu, _), (bl, ll, _) = ops._bones_on(skeleton.WALK_UPPER, L_up, 15, dev, "bench"), ops._bones_on(skeleton.WALK_LOWER, L_lo, 8, dev, "bench")
    ops.blend_windows(win_up, plan, dst[45], spread)                   # (the host check and the upload of the cover happen here, once)
    off, row, w = plan._cover_dev[str(dev)]
    forms = {"blend_windows C = 45 with spread (stride-1 plan)": lambda: hip.call("blend_windows", win_up, n, 45, off, row, w, F, dst[45], 45, spread),
             "blend_windows C = 24 (stride-1 plan)": lambda: hip.call("blend_windows", win_lo, n, 24, off, row, w, F, dst[24], 24, None)}
    for H in HS:
        wd = torch.as_tensor(dense.smooth_weights(H, "gauss")).to(dev)

        def add(H=H, wd=wd):
            forms["smooth_frames C = 45 with moved, H = %d" % H] = lambda: hip.call("smooth_frames", src[45], 45, F, 45, seg, wd, H, 2, dst[45], 45, moved)
            forms["smooth_frames C = 24, H = %d" % H] = lambda: hip.call("smooth_frames", src[24], 24, F, 24, seg, wd, H, 2, dst[24], 24, None)
            forms["smooth_bones J = 15 with moved and fallback, H = %d" % H] = lambda: hip.call(
                "smooth_bones", src[45], 45, F, 15, seg, wd, H, 2, bu, lu, 14, dst[45], 45, moved, fell)
            forms["smooth_bones J = 8, H = %d" % H] = lambda: hip.call("smooth_bones", src[24], 24, F, 8, seg, wd, H, 2, bl, ll, 6, dst[24], 24, None, None)
        add()
    res["launch_us"] = {"F": F, "segments": int(len(np.unique(plan.frame_rec[plan.covered != 0]))), "order": 2, "taper": "gauss",
                        "cover_entries_of_the_blend": int(len(plan.cov_row))}
    res["launch_us"].update(chains_us(forms))
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
        timers["stride %d, smooth" % stride] = timed_pass(stride, smooth=(8, 2, "gauss"))
        timers["stride %d, bones" % stride] = timed_pass(stride, blend_space="bones")
        timers["stride %d, bones, smooth" % stride] = timed_pass(stride, blend_space="bones", smooth=(8, 2, "gauss"))
    for t in timers.values():
        t()
    res["pass_s"] = rounds(timers, 5)
    for stride in (5, 1):
        base_s = res["pass_s"]["stride %d, no argument" % stride]
        band = (max(base_s["rounds"]) - min(base_s["rounds"])) / base_s["median"]
        res["pass_s"]["stride %d: band of the no-argument rounds / median" % stride] = round(band, 4)
        res["pass_s"]["stride %d: smooth / no argument" % stride] = round(res["pass_s"]["stride %d, smooth" % stride]["median"] / base_s["median"], 4)
        res["pass_s"]["stride %d: bones, smooth / bones" % stride] = round(
            res["pass_s"]["stride %d, bones, smooth" % stride]["median"] / res["pass_s"]["stride %d, bones" % stride]["median"], 4)
    print("pass_s", res["pass_s"])

    # (c) the effect
    res["effect_synthetic"] = {"note": "pretrained weights on random clouds against random targets: the figures show the mechanics, not accuracy"}
    keys = ("moved_cm", "accel_cm", "unsmoothed_accel_cm", "all_cm", "unsmoothed_all_cm", "bone_dev_cm")
    for space in ("joints", "bones"):
        for H in HS:
            for order in (0, 1, 2):
                s, _ = dense.dense_infer(base, None, up, lo, ds, 5, batch_size=B, metrics="full", blend_space=space, smooth=(H, order, "gauss"))
                res["effect_synthetic"]["%s H %d order %d gauss" % (space, H, order)] = dict(
                    {k: round(float(s[k]), 5) for k in keys}, smooth_fallback=s["smooth_fallback"])
        s, _ = dense.dense_infer(base, None, up, lo, ds, 5, batch_size=B, metrics="full", blend_space=space, smooth=(8, 2, "box"))
        res["effect_synthetic"]["%s H 8 order 2 box" % space] = dict({k: round(float(s[k]), 5) for k in keys}, smooth_fallback=s["smooth_fallback"])
    print("effect_synthetic", res["effect_synthetic"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "dense_smooth.json")
