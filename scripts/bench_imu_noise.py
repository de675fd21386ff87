"""What --imu_noise_* / --imu_bias_* cost, in ONE process, the variants alternating, three rounds, medians:

  python scripts/bench_imu_noise.py OUT.json [--plain-only | --launch-only]

(a) the mmego_imu_jitter launch alone at 512 rows (B = 64 windows of T = 8 frames of 20 samples: one training minibatch, 614 KB) and at
    32 768 rows (a dense inference pass over a long recording, 39 MB), all six sigmas on, a chain of 16 in one HIP graph, 200 replays;
    at 512 rows also with the additive sigmas only, the two rotation sigmas only and the white rotation only (where the time goes);
(b) the stage-1 training step (ImuStep, IMU_Net of hidden size 512) at B = 64, T = 8, graph replay, on seeded random inputs: without the
    option, and with it and the key rewritten before every step as the trainers do (one int64 fill outside the graph);
(c) the Upper stage training step at B = 64, T = 8, N = 128 with a FROZEN IMU_Net of its own as a plain StageStep (what the stage
    trainers take under the option): without the option and with it;
(d) the same Upper step as PipelinedStages (the frozen forward one minibatch ahead: what the stage trainers take WITHOUT the option): the
    difference to (c) without the option is what giving up the prefetch costs.
--launch-only: (a) alone.  --plain-only: (b), (c) and (d) without the option alone, on code that may not know the option (the parent commit, same session:
MMEGO_BENCH_ROOT names the checkout whose mmego_amd package, built, is imported instead of this one)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.environ.get("MMEGO_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets, ops  # noqa: E402
from mmego_amd.train_step import ImuStep, PipelinedStages, StageStep  # noqa: E402

dev = torch.device("cuda:0")
B, T, N, S = 64, 8, 128, 20
SIGMAS = (1.0, 0.05, 0.01, 2.0, 0.2, 0.02)


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
    imu = torch.randn(B, T, S, 15, generator=g)
    imu[..., :9] = torch.linalg.qr(torch.randn(B, T, S, 3, 3, generator=g))[0].reshape(B, T, S, 9)
    body = torch.randn(B, 20, 3, generator=g) * 0.3
    target = torch.randn(B, T, 21, 3, generator=g)
    R = torch.linalg.qr(torch.randn(B, T, 3, 3, generator=g))[0].contiguous()
    return [v.to(dev) for v in (x, imu, body, target, R)]


def timer(step, rekey=None):
    def ms(n=300, warm=20):
        def one(i):
            if rekey is not None:
                rekey(0x9E3779B97F4A7C15 * (i + 1))
            step()
        for i in range(warm):
            one(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            one(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    return ms


def imu_stepper(**noise):
    torch.manual_seed(1)
    st = ImuStep(nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).train(), lr=1e-4, use_graph=True, **noise)
    x, imu, body, target, R = batch()
    st.bind(imu, R, target)
    return timer(st.step, st.set_imu_key if noise else None)


def upper_stepper(pipelined, **noise):
    torch.manual_seed(1)
    imu_net = nets.IMUNet(15, 9, 512, 2).to(dev).eval()
    up = nets.UpperNet().to(dev).train()
    x, imu, body, target, R = batch()
    if not pipelined:
        st = StageStep("upper", up, imu_net, lr=3e-5, use_graph=True, **noise)
        st.bind(x, imu, body, target)
        return timer(st.step, st.set_imu_key if noise else None)
    st = StageStep("upper", up, None, lr=3e-5, use_graph=False)
    imu_next = imu.clone()
    eng = PipelinedStages([st], [imu_net], imu_next, use_graph=True)
    st.bind(x, imu, body, target)
    eng.prime()
    return timer(eng.step)


def launch_chain(rows, sigmas=SIGMAS):
    g = torch.Generator().manual_seed(rows)
    imu = torch.randn(rows, S, 15, generator=g)
    imu[..., :9] = torch.linalg.qr(torch.randn(rows, S, 3, 3, generator=g))[0].reshape(rows, S, 9)
    imu = imu.to(dev)
    out, word = torch.empty_like(imu), torch.tensor([12345], dtype=torch.int64, device=dev)
    launch = lambda: ops.imu_jitter(imu, sigmas, word, out, T=T)
    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.capture(graph):
        for _ in range(16):
            launch()

    # (the timer keeps the graph's buffers alive: torch.cuda.graph empties the allocator's cache when the NEXT chain is captured, and a
    #  buffer nobody holds any more goes back to the driver under a graph that still points at it)
    def us(reps=200, keep=(imu, out, word)):
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
    res = {"shape": {"B": B, "T": T, "N": N, "S": S}, "imu_noise": list(SIGMAS),
           "method": "step: graph-replayed steps on seeded random inputs, IMU_Net of hidden size 512, 300 steps after 20, wall clock around "
                     "the loop with one synchronisation behind it; launch: a chain of 16 in one HIP graph, 200 replays after 3; the variants "
                     "alternating, three rounds, medians"}
    on = {} if plain_only else {"with": dict(imu_noise=SIGMAS)}
    launch_only = "--launch-only" in sys.argv
    if not plain_only:
        # (the split at 512 rows: the additive groups alone make no rotation -- no sin / cos, no 3 x 3 products -- and the rotations alone
        #  make two per thread)
        res["imu_jitter_launch_us"] = rounds(dict({"%d rows" % n: launch_chain(n) for n in (512, 32768)}, **{
            "512 rows, additive sigmas only": launch_chain(512, (0.0,) + SIGMAS[1:3] + (0.0,) + SIGMAS[4:]),
            "512 rows, rotation sigmas only": launch_chain(512, SIGMAS[:1] + (0.0, 0.0) + SIGMAS[3:4] + (0.0, 0.0)),
            "512 rows, white rotation only": launch_chain(512, SIGMAS[:1] + (0.0,) * 5)}))
        print("imu_jitter_launch_us", res["imu_jitter_launch_us"])
    if launch_only:
        json.dump(res, open(path, "w"), indent=1)
        return
    res["imu_step_ms"] = rounds(dict({"without": imu_stepper()}, **{k + ", key rewritten every step": imu_stepper(**v) for k, v in on.items()}))
    print("imu_step_ms", res["imu_step_ms"])
    res["upper_step_frozen_imu_ms"] = rounds(dict(
        {"plain StageStep, without": upper_stepper(False), "PipelinedStages, without": upper_stepper(True)},
        **{"plain StageStep, " + k + ", key rewritten every step": upper_stepper(False, **v) for k, v in on.items()}))
    print("upper_step_frozen_imu_ms", res["upper_step_frozen_imu_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args[0] if args else "imu_noise.json", "--plain-only" in sys.argv)
