"""What the causal options of dense inference (dense.dense_infer(online=L, one_euro=(fc, beta, dc)): --infer --dense --online
--one_euro FC) cost and change, in ONE process:

  python scripts/bench_dense_online.py OUT.json          (the committed figures: profiles/dense_online.json)

(a) device-event time of the causal filter's launches alone at F = 32 768 frames cut into 256 runs of 128 frames: mmego_one_euro and
    mmego_one_euro_bones at J = 15 (with moved; the bones form with its fallback counts) and J = 8, beta 0 and 10; beside them, as the
    yardstick, mmego_smooth_frames at the same F from the same process (C = 45 with moved, C = 24, H = 8, order 2, gauss); and the same
    F cut into 2048 runs of 16 frames and 32 runs of 1024 -- the launch is one wave per run and sequential along the run, so the run
    LENGTH and not the traffic should set its time -- the forms alternating, 20 chains of 10 calls after 3;
(b) the dense pass, wall clock to its last host read, on Sample_data-shaped synthetic frames (scripts/bench_frame_store.py's generator:
    223 recordings, about 19 100 frames; frame_no 20, window minibatch 64) at stride 1 -- what a streaming device computes: one window
    per frame, frame_no times the windows of the reference's grid -- without the arguments, with online=0, and with online=0 and
    one_euro=(0.05, 10, 0.1); alternating, five rounds, medians, the band of the rounds; and how many windows that is;
(c) what it changes, with the committed pretrained weights on the synthetic frames, --metrics full, stride 1: the joint error, the
    acceleration error and the displacement offline, online at lookahead 0, 4 and 19, and online with the filter at three cutoffs.
    Random clouds and random targets: no error figure says anything about accuracy; the figures show the mechanics only."""
import json
import os
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
from mmego_amd.data import PosePC  # noqa: E402

dev = torch.device("cuda:0")
T, B, F = 20, 64, 32768
EURO = (0.05, 10.0, 0.1)


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
    g = torch.Generator(device=dev).manual_seed(0)
    src = {45: torch.randn((F, 45), device=dev, generator=g), 24: torch.randn((F, 24), device=dev, generator=g)}
    dst = {45: torch.empty((F, 45), device=dev), 24: torch.empty((F, 24), device=dev)}
    moved, fell = torch.empty(F, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
    L_up, L_lo = np.full(14, 0.25, np.float32), np.full(6, 0.4, np.float32)
    (bu, lu, _), (bl, ll, _) = ops._bones_on(skeleton.WALK_UPPER, L_up, 15, dev, "bench"), ops._bones_on(skeleton.WALK_LOWER, L_lo, 8, dev, "bench")
    wd = torch.as_tensor(dense.smooth_weights(8, "gauss")).to(dev)
    res["launch_us"] = {"F": F, "fc": EURO[0], "dc": EURO[2]}
    for R in (256, 2048, 32):
        n = F // R
        seg_h = np.repeat(np.arange(R, dtype=np.int32), n)
        off, on = (torch.as_tensor(a).to(dev) for a in ops.one_euro_runs(seg_h))
        seg = torch.as_tensor(seg_h).to(dev)
        forms = {}
        for beta in (0.0, 10.0):
            def add(beta=beta, off=off, on=on, R=R):
                forms["one_euro J = 15 with moved, beta %g" % beta] = lambda: hip.call(
                    "one_euro", src[45], 45, F, 15, off, on, R, EURO[0], beta, EURO[2], dst[45], 45, moved)
                forms["one_euro J = 8, beta %g" % beta] = lambda: hip.call(
                    "one_euro", src[24], 24, F, 8, off, on, R, EURO[0], beta, EURO[2], dst[24], 24, None)
                forms["one_euro_bones J = 15 with moved and fallback, beta %g" % beta] = lambda: hip.call(
                    "one_euro_bones", src[45], 45, F, 15, off, on, R, EURO[0], beta, EURO[2], bu, lu, 14, dst[45], 45, moved, fell)
                forms["one_euro_bones J = 8, beta %g" % beta] = lambda: hip.call(
                    "one_euro_bones", src[24], 24, F, 8, off, on, R, EURO[0], beta, EURO[2], bl, ll, 6, dst[24], 24, None, None)
            add()
        forms["smooth_frames C = 45 with moved, H = 8"] = lambda seg=seg: hip.call("smooth_frames", src[45], 45, F, 45, seg, wd, 8, 2, dst[45], 45, moved)
        forms["smooth_frames C = 24, H = 8"] = lambda seg=seg: hip.call("smooth_frames", src[24], 24, F, 24, seg, wd, 8, 2, dst[24], 24, None)
        res["launch_us"]["%d runs of %d frames" % (R, n)] = chains_us(forms)
        print("launch_us", R, res["launch_us"]["%d runs of %d frames" % (R, n)])

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
    timers = {"stride 1, no argument": timed_pass(1), "stride 1, online 0": timed_pass(1, online=0),
              "stride 1, online 0, one_euro": timed_pass(1, online=0, one_euro=EURO),
              "stride 1, one_euro": timed_pass(1, one_euro=EURO), "stride 10 (the default), no argument": timed_pass(10)}
    for t in timers.values():
        t()
    res["pass_s"] = rounds(timers, 5)
    base_s = res["pass_s"]["stride 1, no argument"]
    res["pass_s"]["band of the no-argument rounds / median"] = round((max(base_s["rounds"]) - min(base_s["rounds"])) / base_s["median"], 4)
    for k in ("stride 1, online 0", "stride 1, online 0, one_euro", "stride 1, one_euro"):
        res["pass_s"][k + " / no argument"] = round(res["pass_s"][k]["median"] / base_s["median"], 4)
    print("pass_s", res["pass_s"])

    # (c) the effect, and how many windows a streaming device runs
    res["effect_synthetic"] = {"note": "pretrained weights on random clouds against random targets: the figures show the mechanics, not accuracy"}
    keys = ("all_cm", "accel_cm", "spread_cm", "covered_frames", "max_cover", "windows")
    more = ("moved_cm", "unsmoothed_all_cm", "unsmoothed_accel_cm", "one_euro_fallback")
    cases = [("offline", {}, keys)] + [("online %d" % L, dict(online=L), keys + ("warmup_frames",)) for L in (0, 4, 19)]
    cases += [("online 0, one_euro fc %g beta %g" % (fc, beta), dict(online=0, one_euro=(fc, beta, 0.1)), keys + more)
              for fc, beta in ((0.02, 0.0), (0.05, 10.0), (0.5, 10.0))]
    cases += [("online 0, bones, one_euro fc 0.05 beta 10", dict(online=0, blend_space="bones", one_euro=EURO), keys + more + ("bone_dev_cm",))]
    for name, kw, ks in cases:
        s, _ = dense.dense_infer(base, None, up, lo, ds, 1, batch_size=B, metrics="full", **kw)
        res["effect_synthetic"][name] = {k: (s[k] if isinstance(s[k], int) else round(float(s[k]), 5)) for k in ks}
    s10, _ = dense.dense_infer(base, None, up, lo, ds, T, batch_size=B)
    res["windows"] = {"stride 1": res["effect_synthetic"]["offline"]["windows"], "stride frame_no (the reference's grid and a head window)": s10["windows"]}
    print("effect_synthetic", res["effect_synthetic"], res["windows"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "dense_online.json")
