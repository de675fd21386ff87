"""What the learning-rate schedule inside the Adam launch (FusedAdam(lr_schedule=...), --lr_schedule) costs, in ONE process, option off and
on alternating, five rounds, medians and the spread of the rounds beside them:

  python scripts/bench_lr_schedule.py OUT.json

(a) the launches alone, on Upper_Net's flat buffer (0.3 M floats: latency level) and on IMU_Net's (23.1 M): mmego_adam_step against
    mmego_adam_step_sched in its plain form, mmego_adam_step_clipped against the clipped form (its records written once, by one
    mmego_grad_sqnorm), as chains of 16 calls captured into one HIP graph (GPU-side time per call, the dependent launch boundary behind
    each kernel included -- scripts/adam_chain.py).  The schedule is a cosine with warm-up, so every call takes the branch
    with the cos.  Expectation from the code: a handful of double operations in one lane per workgroup, nothing per element -- not
    measurable against the unscheduled launch.
(b) the graph-replayed Upper step (train_step.StageStep, recorded head pose) at B=64, T=8, N=128 without and with the option."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets  # noqa: E402
from adam_chain import CHAIN, ROUNDS, SCHED, Buffers, chain, dev, summary  # noqa: E402

hip.lib()


def launches(n):
    b = Buffers(n)
    timers = {k: chain(b.form(k)) for k in ("adam_step", "adam_step_sched", "adam_step_clipped", "adam_step_sched_clipped")}
    runs = {k: [] for k in timers}
    for _ in range(ROUNDS):
        for k, t in timers.items():
            runs[k].append(round(t(), 3))
    out = {k: summary(v) for k, v in runs.items()}
    out["n"] = n
    for base, with_ in (("adam_step", "adam_step_sched"), ("adam_step_clipped", "adam_step_sched_clipped")):
        out[with_ + "_minus_" + base + "_us"] = round(out[with_]["median"] - out[base]["median"], 3)
        out[base + "_spread_us"] = round(out[base]["max"] - out[base]["min"], 3)
    return out


def upper_step():
    from mmego_amd.train_step import StageStep
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

    def make(sched):
        torch.manual_seed(1)
        st = StageStep("upper", nets.UpperNet().to(dev).train(), None, lr=3e-5, use_graph=True, lr_schedule=sched)
        st.bind(x, imu, body, target, R_gt=Rg)
        return st
    sts = {"off": make(None), "lr_schedule": make(SCHED)}
    runs = {k: [] for k in sts}
    for _ in range(ROUNDS):
        for k, st in sts.items():
            runs[k].append(round(timed(st.step), 4))
    res = {k: summary(v) for k, v in runs.items()}
    res["lr_schedule_minus_off_ms"] = round(res["lr_schedule"]["median"] - res["off"]["median"], 4)
    res["off_spread_ms"] = round(res["off"]["max"] - res["off"]["min"], 4)
    print("upper step", res)
    return {"shape": {"B": B, "T": T, "N": N}, "upper_ms_per_step": res}


def main(path):
    torch.manual_seed(0)
    sizes = {"Upper_Net": nets.UpperNet().to(dev).flat().ensure().flat_p.numel(),
             "IMU_Net": nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).flat().ensure().flat_p.numel()}
    res = {"method": "launches: chains of %d calls in one HIP graph, 20 replays after 3, wall clock per call, the kinds alternating, %d "
                     "rounds; step: graph replay + optimiser launch, 50 steps after 5, option off and on alternating, %d rounds; spread: "
                     "max - min of the unscheduled rounds" % (CHAIN, ROUNDS, ROUNDS),
           "schedule": SCHED.to_dict(), "launch_us": {}}
    for name, n in sizes.items():
        res["launch_us"][name] = launches(n)
        print(name, res["launch_us"][name])
    res.update(upper_step())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "lr_schedule.json")
