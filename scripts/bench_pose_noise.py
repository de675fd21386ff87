"""What --pose_noise_deg / --pose_noise_t cost, in ONE process, the variants alternating, three rounds, medians:

  python scripts/bench_pose_noise.py OUT.json [--plain-only]

(a) the mmego_pose_jitter launch alone at 512 rows (B = 64 windows of T = 8 frames: one training minibatch) and at 32 768 rows (a dense
    inference pass over a long recording), both sigmas on, a chain of 16 in one HIP graph, 200 replays;
(b) the Upper stage training step at B = 64, T = 8, N = 128 with the recorded head pose, graph replay, on seeded random inputs: without
    the option; with it and the key rewritten before every step as the trainers do (one int64 fill outside the graph); and with it and the
    key left alone (the captured launch only) -- which says whether the cost is the node in the graph or the write beside it.
--plain-only: figure (b) without the option alone, on code that may not know the option (the parent commit, same session:
MMEGO_BENCH_ROOT names the checkout whose mmego_amd package, built, is imported instead of this one)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.environ.get("MMEGO_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets, ops  # noqa: E402
from mmego_amd.train_step import StageStep  # noqa: E402

dev = torch.device("cuda:0")
B, T, N = 64, 8, 128
DEG, SHIFT = 2.0, 0.02


def rounds(timers, n=3):
    runs = {k: [] for k in timers}
    for _ in range(n):
        for k, t in timers.items():
            runs[k].append(round(t(), 4))
    return {k: {"rounds": v, "median": statistics.median(v)} for k, v in runs.items()}


def batch(seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, N, 6, generator=g)
    x[:, ::2, 100:] = 0.0
    imu = torch.randn(B, T, 20, 15, generator=g)
    body = torch.randn(B, 20, 3, generator=g) * 0.3
    target = torch.randn(B, T, 21, 3, generator=g)
    R = torch.linalg.qr(torch.randn(B, T, 3, 3, generator=g))[0].contiguous()
    return [v.to(dev) for v in (x, imu, body, target, R)]


def stepper(rekey, **noise):
    torch.manual_seed(1)
    st = StageStep("upper", nets.UpperNet().to(dev).train(), None, lr=3e-5, use_graph=True, **noise)
    x, imu, body, target, R = batch()
    st.bind(x, imu, body, target, R_gt=R)

    def ms(n=500, warm=20):
        def one(i):
            if rekey:
                st.set_pose_key(0x9E3779B97F4A7C15 * (i + 1))
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


def launch_chain(rows):
    g = torch.Generator().manual_seed(rows)
    R = torch.linalg.qr(torch.randn(rows, 3, 3, generator=g))[0].contiguous().to(dev)
    t = torch.randn(rows, 3, generator=g).to(dev)
    Ro, to, word = torch.empty_like(R), torch.empty_like(t), torch.tensor([12345], dtype=torch.int64, device=dev)
    launch = lambda: ops.pose_jitter(R, t, DEG, SHIFT, word, Ro, to)
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


def main(path, plain_only):
    hip.lib()
    res = {"shape": {"B": B, "T": T, "N": N}, "pose_noise_deg": DEG, "pose_noise_t": SHIFT,
           "method": "step: graph-replayed Upper StageStep on seeded random inputs with the recorded head pose, 500 steps after 20, wall clock "
                     "around the loop with one synchronisation behind it; launch: a chain of 16 in one HIP graph, 200 replays after 3; the "
                     "variants alternating, three rounds, medians"}
    if plain_only:
        res["upper_step_ms"] = rounds({"without": stepper(False)})
    else:
        res["pose_jitter_launch_us"] = rounds({"%d rows" % n: launch_chain(n) for n in (512, 32768)})
        print("pose_jitter_launch_us", res["pose_jitter_launch_us"])
        both = dict(pose_noise_deg=DEG, pose_noise_t=SHIFT)
        res["upper_step_ms"] = rounds({"without": stepper(False), "with, key rewritten every step": stepper(True, **both),
                                       "with, key left alone": stepper(False, **both)})
    print("upper_step_ms", res["upper_step_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0] if args else "pose_noise.json", "--plain-only" in sys.argv)
