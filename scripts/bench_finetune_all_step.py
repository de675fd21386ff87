"""Cost of a --finetune_all step (IMU_Net, Upper_Net and Lower_Net trained together, stage 3) at the bench batch B=64, T=8, N=128,
HIP-graph replay, ONE process, beside the two steps it is made of, measured in the same run: stage 1's ImuStep and the --finetune_upper
step on the recorded head pose (train_step).  The three-net body is those two bodies minus the stage-1 loss launch and the recorded-pose
copy, plus what carries the pose gradients (Upper_Net's and Lower_Net's pose shares, one mmego_head_fk_backward_extra), so the yardstick
is the sum of the two -- both of them code paths that exist without the option.  Launch counts per body from a recorded plan.StepPlan.
A fourth body, `imu_around_finetune_upper`, is the control for the ORDER of the work: exactly the launches of those two bodies, on their
own independent nets, with the --finetune_upper body placed between stage 1's forward + loss and its backward -- where the three-net
step has Upper_Net and Lower_Net.  What it costs beyond the sum is what any body of that order costs, whatever the option adds.

  python scripts/bench_finetune_all_step.py [--out profiles/finetune_all_step.json]"""
import collections
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets  # noqa: E402
from mmego_amd.plan import StepPlan  # noqa: E402
from mmego_amd import imu_train, ops  # noqa: E402
from mmego_amd.train_step import ImuStep, StageStep, _Engine  # noqa: E402

dev = torch.device("cuda:0")
hip.lib()
B, T, N = 64, 8, 128
ROUNDS, STEPS = 3, 50
g = torch.Generator().manual_seed(0)
x = torch.randn(B, T, N, 6, generator=g).to(dev)
imu = torch.randn(B, T, 20, 15, generator=g).to(dev)
body = (0.3 * torch.randn(B, 20, 3, generator=g)).to(dev)
target = torch.randn(B, T, 21, 3, generator=g).to(dev)
Rg = torch.linalg.qr(torch.randn(B, T, 3, 3, generator=g))[0].contiguous().to(dev)


def timed(step, n, warm=0):
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


class ImuAroundJoint(_Engine):
    """ImuStep's body with a --finetune_upper body (independent nets, recorded pose) between its forward + loss and its backward."""

    def __init__(self, imu_step, joint, use_graph):
        self.a, self.b, self.use_graph, self.graph = imu_step, joint, use_graph, None

    def _body(self):
        s = self.a.static
        n = s["imu"].shape[0] * s["imu"].shape[1]
        with torch.no_grad():
            ops.copy2d(s["target"].view(n, 63)[:, 60:63], s["head"].view(n, 3))
            R, t = imu_train.forward_train(self.a.net, s["imu"])
            hip.call("imu_loss", R, t, s["R_gt"], s["head"], n, 1.0, self.a.loss, s["dR"], s["dt"])
        self.b._body()
        with torch.no_grad():
            imu_train.backward(self.a.net, s["dR"], s["dt"])

    def _mutable_state(self):
        return self.a._mutable_state() + self.b._mutable_state()

    def _update(self):
        for opt in self.a.optimisers() + self.b.optimisers():
            opt.step()

    def _losses(self):
        return self.a.loss


def make(kind, use_graph=True):
    if kind == "imu_around_finetune_upper":
        return ImuAroundJoint(make("imu", False), make("finetune_upper", False), use_graph)
    torch.manual_seed(1)
    himu = nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).train()
    hup = nets.UpperNet().to(dev).train()
    hlo = nets.LowerNet(64).to(dev).train()
    if kind == "imu":
        st = ImuStep(himu, lr=1e-4, use_graph=use_graph)
        st.bind(imu, Rg, target)
    elif kind == "finetune_upper":
        st = StageStep("lower", hlo, None, upper_frozen=hup, lr=3e-5, use_graph=use_graph, finetune_upper=True, upper_lr=3e-5)
        st.bind(x, None, body, target, R_gt=Rg)
    else:
        st = StageStep("lower", hlo, himu, upper_frozen=hup, lr=3e-5, use_graph=use_graph, finetune_upper=True, upper_lr=3e-5,
                       finetune_imu=True, imu_lr=3e-5)
        st.bind(x, imu, body, target)
    return st


KINDS = ("imu", "finetune_upper", "finetune_all", "imu_around_finetune_upper")
res = {"shape": {"B": B, "T": T, "N": N}, "method": "HIP-graph replay + fused Adam launches, one process; %d interleaved rounds of %d steps "
       "per kind after 10 warm-up steps, wall clock / step; the median round per kind, spread = (max - min) / median of its rounds"
       % (ROUNDS, STEPS), "ms_per_step": {}, "rounds": {k: [] for k in KINDS}, "spread": {}, "launches": {}, "entry_points": {}}
steps = {kind: make(kind) for kind in KINDS}
for kind, st in steps.items():
    st.prepare()
    plan = StepPlan().record(st._body)                      # (recording executes nothing)
    calls = collections.Counter(n for sg in plan.segments for n, _ in sg.calls)
    res["launches"][kind] = sum(calls.values())
    res["entry_points"][kind] = dict(sorted(calls.items(), key=lambda kv: (-kv[1], kv[0])))
    timed(st.step, n=10)
for _ in range(ROUNDS):                                     # interleaved rounds: a drift of the clocks hits every kind alike
    for kind, st in steps.items():
        res["rounds"][kind].append(round(timed(st.step, n=STEPS), 4))
for kind in KINDS:
    r = sorted(res["rounds"][kind])
    res["ms_per_step"][kind] = r[len(r) // 2]
    res["spread"][kind] = round((r[-1] - r[0]) / r[len(r) // 2], 5)
    print("%-15s %.3f ms per step  (rounds: %s, spread %.2f %%; %d launches per body)"
          % (kind, res["ms_per_step"][kind], res["rounds"][kind], 100 * res["spread"][kind], res["launches"][kind]))
ms = res["ms_per_step"]
ms["imu_plus_finetune_upper"] = round(ms["imu"] + ms["finetune_upper"], 4)
res["launches"]["imu_plus_finetune_upper"] = res["launches"]["imu"] + res["launches"]["finetune_upper"]
res["finetune_all_minus_sum_ms"] = round(ms["finetune_all"] - ms["imu_plus_finetune_upper"], 4)
res["finetune_all_minus_sum_rel"] = round(res["finetune_all_minus_sum_ms"] / ms["imu_plus_finetune_upper"], 5)
res["finetune_all_minus_control_ms"] = round(ms["finetune_all"] - ms["imu_around_finetune_upper"], 4)
res["control_minus_sum_ms"] = round(ms["imu_around_finetune_upper"] - ms["imu_plus_finetune_upper"], 4)
parts = collections.Counter(res["entry_points"]["imu"]) + collections.Counter(res["entry_points"]["finetune_upper"])
res["launch_difference"] = {k: res["entry_points"]["finetune_all"].get(k, 0) - parts.get(k, 0)
                            for k in sorted(set(parts) | set(res["entry_points"]["finetune_all"]))
                            if res["entry_points"]["finetune_all"].get(k, 0) != parts.get(k, 0)}
print("finetune_all %.3f ms against imu + finetune_upper %.3f ms: %+.3f ms (%+.2f %%); launches %d against %d; by entry point: %s"
      % (ms["finetune_all"], ms["imu_plus_finetune_upper"], res["finetune_all_minus_sum_ms"], 100 * res["finetune_all_minus_sum_rel"],
         res["launches"]["finetune_all"], res["launches"]["imu_plus_finetune_upper"], res["launch_difference"]))
print("control (the same two bodies' launches in the three-net order) %.3f ms: %+.3f ms over the sum; finetune_all %+.3f ms against it"
      % (ms["imu_around_finetune_upper"], res["control_minus_sum_ms"], res["finetune_all_minus_control_ms"]))
del steps

# where the difference sits: one eager body per kind, every launch between two events, summed per entry point
orig = hip._launch
eager = {}
for kind in KINDS[:3]:
    st = make(kind, use_graph=False)
    for _ in range(3):
        st.step()
    torch.cuda.synchronize()
    rec = collections.defaultdict(list)

    def spy(name, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        orig(name, *a)
        e1.record()
        rec[name].append((e0, e1))

    hip._launch = spy
    try:
        st._body()
        torch.cuda.synchronize()
    finally:
        hip._launch = orig
    eager[kind] = {k: sum(e0.elapsed_time(e1) for e0, e1 in v) for k, v in rec.items()}
    del st
res["eager_body_event_ms"] = {k: round(sum(v.values()), 4) for k, v in eager.items()}
diff = {k: eager["finetune_all"].get(k, 0.0) - eager["imu"].get(k, 0.0) - eager["finetune_upper"].get(k, 0.0)
        for k in set().union(*eager.values())}
res["eager_event_difference_ms"] = {k: round(v, 5) for k, v in sorted(diff.items(), key=lambda kv: -abs(kv[1])) if abs(v) >= 0.002}
res["eager_event_difference_total_ms"] = round(sum(diff.values()), 4)
print("eager bodies, event time: %s; finetune_all - (imu + finetune_upper) = %+.3f ms, by entry point (|d| >= 2 us):"
      % (res["eager_body_event_ms"], res["eager_event_difference_total_ms"]))
for k, v in res["eager_event_difference_ms"].items():
    print("   %-28s %+8.4f ms  (%d launches against %d)" % (k, v, res["entry_points"]["finetune_all"].get(k, 0), parts.get(k, 0)))
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
