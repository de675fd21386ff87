"""What the shaped weight decay inside the Adam launch (FusedAdam(decoupled=..., no_decay=...), --weight_decay / --decay_mode / --no_decay_1d)
costs, in ONE process, option off and on alternating, five rounds, medians and the spread of the rounds beside them:

  python scripts/bench_weight_decay.py OUT.json

(a) the launches alone, on Upper_Net's flat buffer (0.3 M floats: latency level) and on IMU_Net's (23.1 M): mmego_adam_step against
    mmego_adam_step_decay in its plain form -- coupled with a mask, decoupled without one, decoupled with one -- and mmego_adam_step_sched
    against the scheduled decoupled masked form, as chains of 16 calls captured into one HIP graph (scripts/adam_chain.py).  The mask
    alternates runs of 1..70 float4, so both sides of every branch are taken.  Expectation from the bytes: 28 + 1/32 B per parameter
    (0.1 %), one more LDS word, one fmaf per element.
(b) the graph-replayed Upper step (train_step.StageStep, recorded head pose) at B=64, T=8, N=128 without and with the options.

For the plain form against the parent commit's, run scripts/adam_chain.py once per library build, alternating (its docstring)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets  # noqa: E402
from adam_chain import ADAM, CHAIN, ROUNDS, Buffers, chain, dev, summary  # noqa: E402

hip.lib()
# form -> (scheduled, masked, decoupled)
DECAY_FORMS = {"adam_step_decay_l2_masked": (False, True, 0), "adam_step_decay_adamw": (False, False, 1),
               "adam_step_decay_adamw_masked": (False, True, 1), "adam_step_decay_sched_adamw_masked": (True, True, 1)}


def run_mask(n):
    """Runs of 1..70 float4 alternating set and clear, as int64 words on the device."""
    rng = np.random.default_rng(n)
    n4 = n // 4
    lens = rng.integers(1, 71, size=n4 // 35 + 2)
    bits = np.repeat(np.arange(len(lens)) % 2 == 0, lens)[:n4]
    assert len(bits) == n4
    padded = np.zeros((n4 + 63) // 64 * 64, dtype=np.uint8)
    padded[:n4] = bits
    return torch.from_numpy(np.packbits(padded, bitorder="little").view("<i8").copy()).to(dev)


def launches(n):
    b = Buffers(n)
    mask = run_mask(n)

    def decay_form(scheduled, masked, decoupled):
        return lambda: hip.call("adam_step_decay", b.p, b.g, b.m, b.v, b.n, b.state, *ADAM, None, 0, b.ticket, None, 0, 0.0, None, None, 0.0,
                                b.sched if scheduled else None, mask if masked else None, decoupled)
    timers = {k: chain(b.form(k)) for k in ("adam_step", "adam_step_sched")}
    timers.update({k: chain(decay_form(*v)) for k, v in DECAY_FORMS.items()})
    runs = {k: [] for k in timers}
    for _ in range(ROUNDS):
        for k, t in timers.items():
            runs[k].append(round(t(), 3))
    out = {k: summary(v) for k, v in runs.items()}
    out["n"] = n
    for k, (scheduled, _, _) in DECAY_FORMS.items():
        base = "adam_step_sched" if scheduled else "adam_step"
        out[k + "_minus_" + base + "_us"] = round(out[k]["median"] - out[base]["median"], 3)
    for base in ("adam_step", "adam_step_sched"):
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

    def make(**kw):
        torch.manual_seed(1)
        st = StageStep("upper", nets.UpperNet().to(dev).train(), None, lr=3e-5, weight_decay=1e-2, use_graph=True, **kw)
        st.bind(x, imu, body, target, R_gt=Rg)
        return st
    sts = {"off": make(), "adamw_no_decay_1d": make(decoupled=True, no_decay="1d")}
    runs = {k: [] for k in sts}
    for _ in range(ROUNDS):
        for k, st in sts.items():
            runs[k].append(round(timed(st.step), 4))
    res = {k: summary(v) for k, v in runs.items()}
    res["adamw_no_decay_1d_minus_off_ms"] = round(res["adamw_no_decay_1d"]["median"] - res["off"]["median"], 4)
    res["off_spread_ms"] = round(res["off"]["max"] - res["off"]["min"], 4)
    print("upper step", res)
    return {"shape": {"B": B, "T": T, "N": N}, "upper_ms_per_step": res}


def main(path):
    torch.manual_seed(0)
    sizes = {"Upper_Net": nets.UpperNet().to(dev).flat().ensure().flat_p.numel(),
             "IMU_Net": nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).flat().ensure().flat_p.numel()}
    res = {"method": "launches: chains of %d calls in one HIP graph, 20 replays after 3, wall clock per call, the forms alternating, %d "
                     "rounds; step: graph replay + optimiser launch, 50 steps after 5, option off and on alternating, %d rounds; spread: "
                     "max - min of the rounds of the form without the option" % (CHAIN, ROUNDS, ROUNDS),
           "launch_us": {}}
    for name, n in sizes.items():
        res["launch_us"][name] = launches(n)
        print(name, res["launch_us"][name])
    res.update(upper_step())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "weight_decay.json")
