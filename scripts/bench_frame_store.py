"""What the frame-major device store (data.FrameStore: --window_jitter, --point_keep) costs per minibatch against DeviceArrays, in ONE
process, the modes alternating, three rounds, medians:

  python scripts/bench_frame_store.py OUT.json

On Sample_data-shaped synthetic frames (223 recordings, about 19 100 frames, 3 to 174 returns per frame with a median near 77), windows
of T = 8 frames, N = 128 slots, minibatches of B = 64 windows:
(a) one minibatch assembly -- the host's index arithmetic and upload, the gathers / the packing kernel, one synchronisation behind 2 000 calls:
    DeviceArrays.gather (what the parent does), and FrameStore.gather with the options off, with jitter, and with jitter + point_keep 0.8;
    and the packing launch alone (mmego_pack_frames on 512 frames, a chain of 16 in one HIP graph);
(b) an Upper stage training step (recorded head pose, graph-replayed StageStep) fed by each of the same sources: assembly + step."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets, ops  # noqa: E402
from mmego_amd.data import DeviceArrays, FrameStore, PosePC, batch_indices  # noqa: E402

dev = torch.device("cuda:0")
B, T, N = 64, 8, 128


def synthetic_frames(seed=0):
    rng = np.random.default_rng(seed)
    snip = rng.integers(40, 132, 223).astype(np.int64)
    F = int(snip.sum())
    npts = np.clip(np.rint(rng.gamma(6.0, 13.5, F)), 3, 174).astype(np.int64)
    P = int(npts.sum())
    q = np.linalg.qr(rng.normal(size=(F, 3, 3)))[0]
    pts = np.concatenate([rng.normal([0.8, 0.0, 0.2], 0.4, (P, 3)), rng.uniform(10, 46, (P, 1)), rng.normal(0, 0.4, (P, 1))], axis=1)
    return {"pts": pts, "npts": npts, "snip_len": snip, "bones": 0.2 * rng.normal(size=(20, 3)),
            "key": rng.normal(0, 0.4, (F, 21, 3)) + np.array([0.8, 0.0, 0.2]),
            "imu": np.concatenate([np.tile(q.reshape(F, 1, 9), (1, 20, 1)), rng.normal(size=(F, 20, 6))], axis=2),
            "ground": np.zeros((F, 1, 4), np.float32), "foot": np.zeros((F, 2, 2), np.int64), "R": q, "t": np.zeros((F, 1, 3)), "RtW": q}


def rounds(timers, n=3):
    runs = {k: [] for k in timers}
    for _ in range(n):
        for k, t in timers.items():
            runs[k].append(round(t(), 3))
    return {k: {"rounds": v, "median": statistics.median(v)} for k, v in runs.items()}


def main(path):
    hip.lib()
    dec = synthetic_frames()
    PosePC._decode = lambda self: dec
    np.random.seed(0)
    ds = PosePC(train=True, batch_length=T, root=os.path.dirname(os.path.abspath(__file__)), keep_frames=True)
    sources = {"DeviceArrays": DeviceArrays(ds, dev), "FrameStore off": FrameStore(ds, dev),
               "FrameStore jitter": FrameStore(ds, dev, jitter=True, seed=1),
               "FrameStore jitter + point_keep 0.8": FrameStore(ds, dev, jitter=True, point_keep=0.8, seed=1)}
    fs = sources["FrameStore jitter + point_keep 0.8"]
    order = [idx for idx in batch_indices(len(ds), B, True, np.random.RandomState(1234)) if len(idx) == B]
    res = {"shape": {"B": B, "T": T, "N": N}, "frames": int(fs.F), "points": int(dec["npts"].sum()), "training_windows": len(ds),
           "valid_starts": int(len(fs.valid_starts())), "movable_windows": fs.n_movable, "max_points_per_frame": fs.max_n,
           "method": "assembly: 2000 gather() calls (host index + upload + launches) then one synchronisation, wall clock per call, after 50; "
                     "pack launch: a chain of 16 in one HIP graph, 20 replays after 3; step: assembly + graph-replayed Upper StageStep, 500 "
                     "after 20; the sources alternating, three rounds, medians"}

    def assembly(src):
        def us(n=2000, warm=50):
            for i in range(warm):
                src.gather(order[i % len(order)])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                src.gather(order[i % len(order)])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e6
        return us
    res["assembly_us"] = rounds({k: assembly(s) for k, s in sources.items()})
    print("assembly_us", res["assembly_us"])

    # the packing launch alone
    fidx = torch.as_tensor(fs.frame_index(order[0])).to(dev)
    out = torch.empty((B * T, N, 6), device=dev)
    launch = lambda: ops.pack_frames(fs.pts, fs.off, fidx, out, fs.max_n, 0.8, 7)
    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.capture(graph):
        for _ in range(16):
            launch()

    def pack_us(reps=20):
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            graph.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (reps * 16) * 1e6
    res["pack_frames_launch_us"] = rounds({"512 frames": pack_us})["512 frames"]
    print("pack_frames_launch_us", res["pack_frames_launch_us"])

    # an Upper stage step fed by each source
    from mmego_amd.train_step import StageStep
    def stepper(src):
        torch.manual_seed(1)
        st = StageStep("upper", nets.UpperNet().to(dev).train(), None, lr=3e-5, use_graph=True)      # (one engine per source: bound once)

        def ms(n=500, warm=20):
            def one(i):
                b = src.gather(order[i % len(order)])
                if st.static is None or st.static["x_src"].data_ptr() != b["data"].data_ptr():
                    st.bind(b["data"], b["imu"], b["skl"], b["target"], R_gt=b["R_R0R"])
                st.step()
            for i in range(warm):
                one(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                one(i)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3
        return ms
    res["upper_step_ms"] = rounds({k: stepper(s) for k, s in sources.items()})
    print("upper_step_ms", res["upper_step_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "frame_store.json")
