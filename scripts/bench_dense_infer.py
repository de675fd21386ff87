"""What dense inference (dense.dense_infer: --infer --dense) costs and shows, in ONE process, three rounds, medians:

  python scripts/bench_dense_infer.py OUT.json

(a) the dense pass, wall clock to its last host read, on Sample_data-shaped synthetic frames (scripts/bench_frame_store.py's generator:
    223 recordings, about 19 100 frames; frame_no 20, window minibatch 64) at strides 20, 10, 5 and 1, beside the yardstick: the plain
    evaluate_full pass over the reference's windows at B = 1 and B = 64 -- windows per second, and the time per window over the yardstick's;
    the plan + upload (DenseWindows' constructor) on its own;
(b) device-event time of the two new launches at the largest shape of the real layout (tests/golden/g11_loader.npz, stride 1: 19 114
    frames, 14 877 windows, cover up to 20): mmego_blend_windows at C = 45 with spread, mmego_colsum_phase over 14 877 x 20 rows of 43
    columns; bytes the algorithm needs over that time, against the 8 TB/s HBM peak;
(c) the window-edge effect with the committed pretrained weights: the error by window position on the 16 committed real windows
    (tests/golden/real16.npz -- the only real sequences at hand: 16 windows of exactly 20 frames, so nothing to blend there), and blended
    against single-window error for both blends on the synthetic frames (random clouds: only the mechanics, no accuracy claim)."""
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
from mmego_amd import dense, hip, nets, ops, processors  # noqa: E402
from mmego_amd.config import ConfigDemo  # noqa: E402
from mmego_amd.data import ArraySplit, DensePlan, DenseWindows, PosePC  # noqa: E402
from mmego_amd.train_step import call_upper  # noqa: E402

dev = torch.device("cuda:0")
T, B = 20, 64
HBM_PEAK = 8.0e12


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


def load(module, npz):
    module.load_state_dict({k: torch.tensor(npz[k]) for k in npz.files})
    return module.to(dev).eval()


def event_us(launch, reps=20, warm=3):
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return {"median": round(statistics.median(times), 2), "min": round(min(times), 2), "max": round(max(times), 2)}


def main(path):
    hip.lib()
    ConfigDemo.gt_head_pose = True
    base = processors._Base(ConfigDemo, make_dirs=False)
    up, lo = load(nets.UpperNet(), golden("w_upper_pretrained.npz")), load(nets.LowerNet(64), golden("w_lower_pretrained.npz"))
    dec = synthetic_frames()
    PosePC._decode = lambda self: dec
    np.random.seed(0)
    ds = PosePC(train=False, vis=True, batch_length=T, root=os.path.join(ROOT, "scripts"), keep_frames=True)
    res = {"shape": {"frame_no": T, "window_minibatch": B}, "frames": int(len(ds.frame_npts_)), "reference_windows": len(ds),
           "method": "wall clock around a whole pass (its last statement is a device -> host read), one warm pass each, then the passes "
                     "alternating, three rounds, medians; launches: device events around one launch, 20 after 3"}

    # (a) the pass
    def timed_pass(stride):
        def s():
            t0 = time.perf_counter()
            dense.dense_infer(base, None, up, lo, ds, stride, batch_size=B)
            return time.perf_counter() - t0
        return s

    def plain(bs):
        def s():
            t0 = time.perf_counter()
            processors.evaluate_full(base, None, up, lo, ds, bs, False)
            return time.perf_counter() - t0
        return s

    def plan_only():
        t0 = time.perf_counter()
        DenseWindows(ds, dev, 1)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    timers = {"evaluate_full B=1": plain(1), "evaluate_full B=64": plain(B)}
    timers.update({"dense stride %d" % s: timed_pass(s) for s in (20, 10, 5, 1)})
    timers["plan + upload (stride 1)"] = plan_only
    for t in timers.values():
        t()                                                        # (warm: every minibatch size's first launches, the device copies)
    res["pass_s"] = rounds(timers)
    lengths = np.bincount(ds.frame_rec_)
    windows = {"evaluate_full B=1": len(ds), "evaluate_full B=64": len(ds)}
    windows.update({"dense stride %d" % s: DensePlan(lengths, T, s).W for s in (20, 10, 5, 1)})
    res["windows"] = windows
    res["windows_per_s"] = {k: round(n / res["pass_s"][k]["median"], 1) for k, n in windows.items()}
    per_window = {k: res["pass_s"][k]["median"] / n for k, n in windows.items()}
    res["time_per_window_over_evaluate_full_B64"] = {k: round(v / per_window["evaluate_full B=64"], 3) for k, v in per_window.items()}
    res["time_per_window_over_evaluate_full_B1"] = {k: round(v / per_window["evaluate_full B=1"], 3) for k, v in per_window.items()}
    print("pass_s", res["pass_s"], "\nwindows_per_s", res["windows_per_s"])

    # (b) the launches at the largest shape
    plan = DensePlan(golden("g11_loader.npz")["dec.snip_len"].astype(np.int64), T, 1)
    g = torch.Generator(device=dev).manual_seed(0)
    src = torch.randn((plan.W * T, 45), device=dev, generator=g)
    dst, spread = torch.empty((plan.F, 45), device=dev), torch.empty(plan.F, device=dev)
    E, pos = torch.rand((plan.W * T, 43), device=dev, generator=g), torch.empty((T, 43), device=dev)
    nnz = len(plan.cov_row)
    blend_bytes = nnz * 45 * 4 + nnz * 8 + (plan.F + 1) * 8 + plan.F * 46 * 4
    phase_bytes = plan.W * T * 43 * 4 + T * 43 * 4
    ops.blend_windows(src, plan, dst, spread)                      # (the cover's host check and upload happen here, once)
    off, row, w = plan._cover_dev[str(dev)]
    bl = event_us(lambda: hip.call("blend_windows", src, plan.W * T, 45, off, row, w, plan.F, dst, 45, spread))
    bl_plain = event_us(lambda: hip.call("blend_windows", src, plan.W * T, 45, off, row, w, plan.F, dst, 45, None))
    ph = event_us(lambda: ops.colsum_phase(E, T, pos))
    res["launch_us"] = {
        "blend_windows F=%d C=45 cover<=%d, with spread" % (plan.F, plan.max_cover): dict(bl, bytes=blend_bytes, tb_per_s=round(blend_bytes / bl["median"] / 1e6, 3), share_of_hbm_peak=round(blend_bytes / bl["median"] * 1e6 / HBM_PEAK, 4)),
        "blend_windows, without spread": dict(bl_plain, bytes=blend_bytes - plan.F * 4, tb_per_s=round(blend_bytes / bl_plain["median"] / 1e6, 3), share_of_hbm_peak=round(blend_bytes / bl_plain["median"] * 1e6 / HBM_PEAK, 4)),
        "colsum_phase %d x %d rows, C=43" % (plan.W, T): dict(ph, bytes=phase_bytes, tb_per_s=round(phase_bytes / ph["median"] / 1e6, 3), share_of_hbm_peak=round(phase_bytes / ph["median"] * 1e6 / HBM_PEAK, 4))}
    print("launch_us", res["launch_us"])

    # (c) the edge effect
    real = golden("real16.npz")
    split = ArraySplit(real["x"], real["target"], real["skl"], real["imu"], real["R"])
    n = len(split)
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)
    win_up, win_lo = torch.empty((n * T, 45), device=dev), torch.empty((n * T, 24), device=dev)
    h0, c0 = torch.zeros((6, 1, 64), device=dev), torch.zeros((6, 1, 64), device=dev)
    with torch.no_grad():
        for i in range(n):
            x, tgt, skl = f32(real["x"][i:i + 1]), f32(real["target"][i:i + 1]), f32(real["skl"][i:i + 1])
            R, t = base.head_pose(None, None, f32(real["R"][i:i + 1]), tgt)
            u = call_upper(up, x, h0, c0, skl, R, t)[0]
            l, _ = lo(u.clone(), x, h0, h0, h0, h0, skl, R, t)
            win_up[i * T:(i + 1) * T].copy_(u.reshape(T, 45))
            win_lo[i * T:(i + 1) * T].copy_(l.reshape(T, 24))
        Er = torch.empty((n * T, 43), device=dev)
        hip.call("pose_errors", win_up, win_lo, f32(real["target"]).reshape(n * T, 63), n * T, Er)
        posr = torch.empty((T, 43), device=dev)
        ops.colsum_phase(Er, T, posr)
    position = posr.cpu().numpy().astype(np.float64)[:, :21].mean(axis=1) / n * 100
    res["edge_effect_real16"] = {"windows": n, "position_cm": [round(float(v), 4) for v in position], "all_cm": round(float(position.mean()), 4),
                                 "ends_cm (positions 0, 19)": round(float(position[[0, -1]].mean()), 4),
                                 "middle_cm (positions 5..14)": round(float(position[5:15].mean()), 4)}
    print("edge_effect_real16", res["edge_effect_real16"])
    res["blend_against_single_synthetic"] = {}
    for blend in ("mean", "triangle"):
        for stride in (10, 5, 1):
            s, _ = dense.dense_infer(base, None, up, lo, ds, stride, blend=blend, batch_size=B, metrics="full")
            res["blend_against_single_synthetic"]["%s stride %d" % (blend, stride)] = {
                "blended_all_cm": round(s["all_cm"], 4), "single_all_cm": round(s["single_all_cm"], 4), "spread_cm": round(s["spread_cm"], 4),
                "accel_cm": round(s["accel_cm"], 4), "position_cm": [round(float(v), 4) for v in s["position_cm"]]}
    s, _ = dense.dense_infer(base, None, up, lo, ds, T, batch_size=B, metrics="full")
    res["blend_against_single_synthetic"]["mean stride 20"] = {
        "blended_all_cm": round(s["all_cm"], 4), "single_all_cm": round(s["single_all_cm"], 4), "accel_cm": round(s["accel_cm"], 4),
        "single_accel_cm (stitched reference windows)": round(s["single_accel_cm"], 4)}
    print("blend_against_single_synthetic", {k: {a: b for a, b in v.items() if a != "position_cm"} for k, v in res["blend_against_single_synthetic"].items()})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "dense_infer.json")
