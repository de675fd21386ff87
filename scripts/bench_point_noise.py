"""What --point_noise / --point_noise_v cost on top of the packing they ride on (data.FrameStore under --point_keep), by the method
and on the synthetic frames of scripts/bench_frame_store.py, in ONE process, the sources alternating, three rounds, medians:

  python scripts/bench_point_noise.py OUT.json

B = 64 windows of T = 8 frames, N = 128 slots; FrameStore with point_keep 0.8 against the same store with point_noise 0.02 and
point_noise_v 0.1 as well, each with and without window jitter (the recorded figures of profiles/frame_store.json are with jitter):
(a) one minibatch assembly (2 000 gather() calls, one synchronisation behind them);
(b) the packing launch alone on 512 frames, a chain of 16 in one HIP graph, 200 replays: mmego_pack_frames, and mmego_pack_frames_noise with the
    velocity's sigma only (4 hashes per kept return), x, y, z only (12) and both (16);
(c) an Upper stage training step fed by each source: assembly + step."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_frame_store import B, N, T, dev, rounds, synthetic_frames  # noqa: E402
from mmego_amd import hip, nets, ops  # noqa: E402
from mmego_amd.data import FrameStore, PosePC, batch_indices  # noqa: E402

KEEP, SIGMA_XYZ, SIGMA_V = 0.8, 0.02, 0.1


def main(path):
    hip.lib()
    dec = synthetic_frames()
    PosePC._decode = lambda self: dec
    np.random.seed(0)
    ds = PosePC(train=True, batch_length=T, root=os.path.dirname(os.path.abspath(__file__)), keep_frames=True)
    noise = dict(point_noise=SIGMA_XYZ, point_noise_v=SIGMA_V)
    sources = {"point_keep 0.8": FrameStore(ds, dev, point_keep=KEEP, seed=1),
               "point_keep 0.8 + noise": FrameStore(ds, dev, point_keep=KEEP, seed=1, **noise),
               "jitter + point_keep 0.8": FrameStore(ds, dev, jitter=True, point_keep=KEEP, seed=1),
               "jitter + point_keep 0.8 + noise": FrameStore(ds, dev, jitter=True, point_keep=KEEP, seed=1, **noise)}
    fs = sources["point_keep 0.8 + noise"]
    order = [idx for idx in batch_indices(len(ds), B, True, np.random.RandomState(1234)) if len(idx) == B]
    res = {"shape": {"B": B, "T": T, "N": N}, "frames": int(fs.F), "points": int(dec["npts"].sum()), "max_points_per_frame": fs.max_n,
           "point_keep": KEEP, "point_noise": SIGMA_XYZ, "point_noise_v": SIGMA_V,
           "recorded": {"source": "profiles/frame_store.json, FrameStore jitter + point_keep 0.8", "assembly_us": 72.577, "upper_step_ms": 0.546,
                        "pack_frames_launch_us": 17.577},
           "method": "as scripts/bench_frame_store.py -- assembly: 2000 gather() calls then one synchronisation, wall clock per call, after 50; "
                     "pack launch: a chain of 16 in one HIP graph, 200 replays after 3 (a window ten times the sibling's); step: assembly + graph-replayed Upper StageStep, 500 "
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

    def chain(launch):
        launch()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with ops.capture(graph):
            for _ in range(16):
                launch()

        def us(reps=200):
            for _ in range(3):
                graph.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                graph.replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / (reps * 16) * 1e6
        return us
    noisy = lambda sx, sv: lambda: ops.pack_frames_noise(fs.pts, fs.off, fidx, out, fs.max_n, KEEP, 7, sx, sv)
    res["pack_launch_us"] = rounds({"pack_frames": chain(lambda: ops.pack_frames(fs.pts, fs.off, fidx, out, fs.max_n, KEEP, 7)),
                                    "pack_frames_noise velocity": chain(noisy(0.0, SIGMA_V)),
                                    "pack_frames_noise xyz": chain(noisy(SIGMA_XYZ, 0.0)),
                                    "pack_frames_noise xyz + velocity": chain(noisy(SIGMA_XYZ, SIGMA_V))})
    res["kept_returns_per_launch"] = int((out[..., 5] != 0).sum())
    print("pack_launch_us", res["pack_launch_us"])

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
    main(sys.argv[1] if len(sys.argv) > 1 else "point_noise.json")
