"""What the weight average (FusedAdam(ema_decay=...), --ema_decay) costs, in ONE process, flag off and flag on alternating, three
rounds, medians:

  python scripts/bench_ema_step.py OUT.json

(a) the launches alone, on IMU_Net's flat buffer (23.1 M floats), on Upper_Net's (0.3 M: latency level) and on one four times IMU_Net's
    (92.5 M: no buffer of either form survives in the Infinity Cache from one launch of the chain to the next): mmego_adam_step against
    mmego_adam_step_ema and mmego_adam_step_clipped against mmego_adam_step_clipped_ema (the update launch of the clipping pair; its
    records are written once, by one mmego_grad_sqnorm), as chains of 16 calls captured into one HIP graph (GPU-side time per call, the
    dependent launch boundary behind each kernel included -- scripts/adam_chain.py).  The boundary itself: the same chain
    of plain steps on 4 floats.
    Yardstick, from the launch without the average measured in the same process: with <= without + (without - boundary) * 8 / 28 -- the
    time the launch's own achieved byte rate needs for 8 more bytes per parameter (28 B/param without, 36 with: the average is read
    and written once).
(b) the graph-replayed stage-1 step (train_step.ImuStep) and the --finetune_imu step (train_step.StageStep) at B=64, T=8, N=128, without
    and with ema_decay (both optimisers of the fine-tuning step average)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets  # noqa: E402
from adam_chain import CHAIN, DECAY, Buffers, chain, dev  # noqa: E402

hip.lib()


def launches(n):
    b, tiny = Buffers(n), Buffers(4)
    timers = dict({"boundary": chain(tiny.form("adam_step"))},
                  **{k: chain(b.form(k)) for k in ("adam_step", "adam_step_ema", "adam_step_clipped", "adam_step_clipped_ema")})
    runs = {k: [] for k in timers}
    for _ in range(3):
        for k, t in timers.items():
            runs[k].append(round(t(), 3))
    out = {k: {"rounds": v, "median": statistics.median(v)} for k, v in runs.items()}
    bd = out["boundary"]["median"]
    out["n"] = n

    def rate(nbytes, us):                                              # TB/s of the time above the boundary; None at latency level
        return round(nbytes / (us - bd) / 1e6, 3) if us > 2 * bd else None
    for base in ("adam_step", "adam_step_clipped"):
        without, with_ = out[base]["median"], out[base + "_ema"]["median"]
        out[base + "_TBps"], out[base + "_ema_TBps"] = rate(28 * n, without), rate(36 * n, with_)
        out[base + "_ema_yardstick_us"] = round(without + (without - bd) * 8 / 28, 3)
        out[base + "_ema_over_yardstick_us"] = round(with_ - out[base + "_ema_yardstick_us"], 3)
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

    def make(kind, decay):
        torch.manual_seed(1)
        himu = nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).train()
        if kind == "stage1":
            st = ImuStep(himu, lr=1e-4, use_graph=True, ema_decay=decay)
            st.bind(imu, Rg, target)
        else:
            st = StageStep("upper", nets.UpperNet().to(dev).train(), himu, lr=3e-5, use_graph=True, finetune_imu=True, imu_lr=3e-5,
                           ema_decay=decay)
            st.bind(x, imu, body, target)
        return st
    res = {}
    for kind in ("stage1", "finetune"):
        sts = {decay: make(kind, decay) for decay in (None, DECAY)}
        runs = {decay: [] for decay in sts}
        for _ in range(3):
            for decay, st in sts.items():
                runs[decay].append(round(timed(st.step), 4))
        res[kind] = {("off" if decay is None else "ema_decay=%g" % decay): {"rounds": v, "median": statistics.median(v)}
                     for decay, v in runs.items()}
        print(kind, res[kind])
        del sts
    return {"shape": {"B": B, "T": T, "N": N}, "ms_per_step": res}


def main(path):
    torch.manual_seed(0)
    sizes = {"IMU_Net": nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).flat().ensure().flat_p.numel(),
             "Upper_Net": nets.UpperNet().to(dev).flat().ensure().flat_p.numel()}
    res = {"method": "launches: chains of %d calls in one HIP graph, 20 replays after 3, wall clock per call, the kinds alternating, three "
                     "rounds; steps: graph replay + optimiser launches, 50 steps after 5, flag off and on alternating, three rounds" % CHAIN,
           "ema_decay": DECAY, "launch_us": {}}
    # (IMU_Net's four buffers are 370 MB and its five 462 MB against 256 MB of Infinity Cache, which a chain of launches over the same
    #  buffers partly lives in; at four times the size -- 1.5 and 1.8 GB -- neither form finds anything there)
    sizes["IMU_Net_x4"] = 4 * sizes["IMU_Net"]
    for name, n in sizes.items():
        res["launch_us"][name] = launches(n)
        print(name, res["launch_us"][name])
    res.update(steps())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "ema_step.json")
