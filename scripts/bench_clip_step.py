"""What global-norm gradient clipping (FusedAdam(max_grad_norm=...), --clip_grad_norm) costs, in ONE process, flag off and flag on
alternating, three rounds, medians:

  python scripts/bench_clip_step.py OUT.json

(a) the launches alone, on IMU_Net's flat buffer (23.1 M floats: the net this is for) and on Upper_Net's (0.3 M: latency level): the
    plain mmego_adam_step, the pair mmego_grad_sqnorm + mmego_adam_step_clipped, and each half of the pair, as chains of 16 calls captured
    into one HIP graph (GPU-side time per call, the dependent launch boundary behind each kernel included; an event pair around ONE
    launch bottoms out near 15 us here and cannot tell these apart).  The boundary itself: the same chain of plain steps on 4 floats (one
    workgroup, one lane at work).
    Yardstick, from the plain launch measured in the same process: pair <= plain + (plain - boundary) * 4 / 28 + boundary -- the plain
    launch, the time its own achieved byte rate needs for 4 more bytes per parameter (28 B/param today), one more dependent boundary.
(b) the graph-replayed stage-1 step (train_step.ImuStep) and the --finetune_imu step (train_step.StageStep) at B=64, T=8, N=128, without
    and with clip_grad_norm (both optimisers of the fine-tuning step clip)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets  # noqa: E402
from adam_chain import CHAIN, Buffers, chain, dev  # noqa: E402

hip.lib()


def launches(n):
    b, tiny = Buffers(n), Buffers(4)
    timers = {"boundary": chain(tiny.form("adam_step")), "plain": chain(b.form("adam_step")), "pair": chain(b.pair),
              "grad_sqnorm": chain(b.norm), "adam_step_clipped": chain(b.form("adam_step_clipped"))}
    runs = {k: [] for k in timers}
    for _ in range(3):
        for k, t in timers.items():
            runs[k].append(round(t(), 3))
    out = {k: {"rounds": v, "median": statistics.median(v)} for k, v in runs.items()}
    plain, pair, bd = (out[k]["median"] for k in ("plain", "pair", "boundary"))
    out["n"] = n
    out["records"] = b.part.numel()
    def rate(nbytes, us):                                              # TB/s of the time above the boundary; None at latency level
        return round(nbytes / (us - bd) / 1e6, 3) if us > 2 * bd else None
    out["plain_TBps"] = rate(28 * n, plain)
    out["grad_sqnorm_TBps"] = rate(4 * n, out["grad_sqnorm"]["median"])
    out["yardstick_us"] = round(plain + (plain - bd) * 4 / 28 + bd, 3)
    out["pair_over_yardstick_us"] = round(pair - out["yardstick_us"], 3)
    return out


def steps():
    from mmego_amd.train_step import ImuStep, StageStep
    B, T, N = 64, 8, 128
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, N, 6, generator=g).to(dev)
    imu = torch.randn(B, T, 20, 15, generator=g).to(dev)
    body = (0.3 * torch.randn(B, 20, 3, generator=g)).to(dev)
    target = torch.randn(B, T, 21, 3, generator=g).to(dev)
    Rg = torch.linalg.qr(torch.randn(B, T, 3, 3, generator=g))[0].contiguous().to(dev)

    def timed(step, n=50, warm=5):
        for _ in range(warm):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def make(kind, clip):
        torch.manual_seed(1)
        himu = nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).train()
        if kind == "stage1":
            st = ImuStep(himu, lr=1e-4, use_graph=True, clip_grad_norm=clip)
            st.bind(imu, Rg, target)
        else:
            st = StageStep("upper", nets.UpperNet().to(dev).train(), himu, lr=3e-5, use_graph=True, finetune_imu=True, imu_lr=3e-5,
                           clip_grad_norm=clip)
            st.bind(x, imu, body, target)
        return st
    res = {}
    for kind in ("stage1", "finetune"):
        sts = {clip: make(kind, clip) for clip in (None, 1.0)}
        runs = {clip: [] for clip in sts}
        for _ in range(3):
            for clip, st in sts.items():
                runs[clip].append(round(timed(st.step), 4))
        res[kind] = {("off" if clip is None else "clip_grad_norm=%g" % clip): {"rounds": v, "median": statistics.median(v)}
                     for clip, v in runs.items()}
        res[kind]["stats"] = {n: getattr(sts[1.0], n).grad_stats() for n in ("opt", "imu_opt") if getattr(sts[1.0], n, None) is not None}
        print(kind, res[kind])
        del sts
    return {"shape": {"B": B, "T": T, "N": N}, "ms_per_step": res}


def main(path):
    torch.manual_seed(0)
    sizes = {"IMU_Net": nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).flat().ensure().flat_p.numel(),
             "Upper_Net": nets.UpperNet().to(dev).flat().ensure().flat_p.numel()}
    res = {"method": "launches: chains of %d calls in one HIP graph, 20 replays after 3, wall clock per call, the kinds alternating, three "
                     "rounds; steps: graph replay + optimiser launches, 50 steps after 5, flag off and on alternating, three rounds" % CHAIN,
           "launch_us": {}}
    for name, n in sizes.items():
        res["launch_us"][name] = launches(n)
        print(name, res["launch_us"][name])
    res.update(steps())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "clip_grad_norm_step.json")
