"""The fused Adam step's launches alone, timed as chains of 16 calls captured into one HIP graph: GPU-side time per call, the dependent
launch boundary behind each kernel included (an event pair around ONE launch bottoms out near 15 us here and cannot tell the forms
apart).  bench_clip_step.py, bench_ema_step.py and bench_lr_schedule.py take `Buffers` and `chain` from here.

Run as a program it times the eight forms of csrc/optim.hip's step (clipped or not, averaged or not, scheduled or not) on Upper_Net's
flat buffer (299 660 floats: latency level) and IMU_Net's (23 119 920), the forms alternating, five rounds, median and min-max per form:

  MMEGO_HIP_LIB=<library> python scripts/adam_chain.py OUT.json

For an A/B of two library builds run it once per library, alternating, several times: the min-max range of one library's rounds over
all its runs is what the method resolves."""
import functools
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, ops  # noqa: E402
from mmego_amd.params import LrSchedule  # noqa: E402

dev = torch.device("cuda:0")
ADAM = (3e-5, 0.9, 0.999, 1e-8, 1e-3)
DECAY = 0.999
MAX_NORM = 1.0
SCHED = LrSchedule("cosine", warmup=100, span=100000, floor=0.1)       # (every call takes the branch with the cos)
CHAIN, ROUNDS = 16, 5
# form -> (clipped, averaged, scheduled)
FORMS = {"adam_step" + ("_sched" if s else "") + ("_clipped" if c else "") + ("_ema" if e else ""): (c, e, s)
         for s in (False, True) for c in (False, True) for e in (False, True)}
SIZES = {"Upper_Net": 299660, "IMU_Net": 23119920}


class Buffers:
    """One optimiser's buffers for n floats; the records of the clipped forms are written once, here."""

    def __init__(self, n):
        g = torch.Generator(device=dev).manual_seed(n)
        self.n = n
        self.p, self.g = torch.randn(n, device=dev, generator=g), torch.randn(n, device=dev, generator=g) * 0.01
        self.m, self.v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        self.ema = self.p.clone()
        self.state = torch.zeros(4, dtype=torch.float64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.part = torch.zeros(hip.lib().mmego_grad_norm_nblk(n), dtype=torch.float64, device=dev)
        self.stats = torch.zeros(8, dtype=torch.float64, device=dev)
        self.sched = SCHED.c_struct()
        self.norm()

    def norm(self):
        hip.call("grad_sqnorm", self.g, self.n, None, 0, self.part, self.part.numel())

    def step(self, clipped, averaged, scheduled):
        common = (self.p, self.g, self.m, self.v, self.n, self.state, *ADAM, None, 0, self.ticket)
        clip = (self.part, self.part.numel(), MAX_NORM, self.stats) if clipped else ()
        avg = (self.ema, DECAY) if averaged else ()
        if scheduled:
            hip.call("adam_step_sched", *common, *(clip or (None, 0, 0.0, None)), *(avg or (None, 0.0)), self.sched)
        else:
            hip.call("adam_step" + ("_clipped" if clipped else "") + ("_ema" if averaged else ""), *common, *clip, *avg)

    def form(self, name):
        """The launch of one of FORMS as a function without arguments."""
        return functools.partial(self.step, *FORMS[name])

    def pair(self):
        self.norm()
        self.step(True, False, False)


def chain(fn):
    """fn CHAIN times in a row as one HIP graph -> a function returning the GPU-side us per call (20 replays, wall clock)."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.capture(graph):
        for _ in range(CHAIN):
            fn()

    def us(reps=20):
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            graph.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (reps * CHAIN) * 1e6
    return us


def summary(v):
    return {"rounds": v, "median": statistics.median(v), "min": min(v), "max": max(v)}


def main(path):
    hip.lib()
    res = {"method": "chains of %d calls in one HIP graph, 20 replays after 3, wall clock per call, the forms alternating, %d rounds"
                     % (CHAIN, ROUNDS), "library": hip.LIBPATH, "launch_us": {}}
    for name, n in SIZES.items():
        b = Buffers(n)
        timers = {form: chain(b.form(form)) for form in FORMS}
        runs = {form: [] for form in FORMS}
        for _ in range(ROUNDS):
            for form, t in timers.items():
                runs[form].append(round(t(), 3))
        res["launch_us"][name] = dict({form: summary(v) for form, v in runs.items()}, n=n)
        for form, v in runs.items():
            print("%-10s %-30s %9.3f us  (%.3f - %.3f)" % (name, form, statistics.median(v), min(v), max(v)))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "adam_chain.json")
