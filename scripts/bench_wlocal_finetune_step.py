"""Cost of a --finetune_imu step around UpperNetwlocal (--upper_variant wlocal: IMU_Net and UpperNetwlocal trained end to end) at the bench
batch B=64, T=8, N=128, HIP-graph replay, ONE process, beside the two steps it is made of, measured in the same run: stage 1's ImuStep and
the plain UpperNetwlocal step on the recorded head pose (train_step) -- both code paths that exist without the option, so the yardstick
is their sum.  The fine-tuning body is those two bodies minus the stage-1 loss launch and the recorded-pose copies, plus what carries the
pose gradients (mmego_head_fk_loss_pose for mmego_head_fk_loss, one mmego_transform2h_backward).  Launch counts per body from a
recorded plan.StepPlan.  Protocol of scripts/bench_finetune_all_step.py: interleaved rounds, the median round per kind.

  python scripts/bench_wlocal_finetune_step.py [--out profiles/wlocal_finetune_step.json]"""
import collections
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets, nets_local  # noqa: E402
from mmego_amd.plan import StepPlan  # noqa: E402
from mmego_amd.train_step import ImuStep, StageStep  # noqa: E402

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


def timed(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def make(kind):
    torch.manual_seed(1)
    himu = nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).train()
    hup = nets_local.UpperNetwlocal().to(dev).train()
    if kind == "imu":
        st = ImuStep(himu, lr=1e-4, use_graph=True)
        st.bind(imu, Rg, target)
    elif kind == "wlocal_recorded_pose":
        st = StageStep("upper", hup, None, lr=3e-5, use_graph=True)
        st.bind(x, imu, body, target, R_gt=Rg)
    else:
        st = StageStep("upper", hup, himu, lr=3e-5, use_graph=True, finetune_imu=True, imu_lr=3e-5)
        st.bind(x, imu, body, target)
    return st


KINDS = ("imu", "wlocal_recorded_pose", "wlocal_finetune_imu")
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
    print("%-22s %.3f ms per step  (rounds: %s, spread %.2f %%; %d launches per body)"
          % (kind, res["ms_per_step"][kind], res["rounds"][kind], 100 * res["spread"][kind], res["launches"][kind]))
ms = res["ms_per_step"]
ms["imu_plus_wlocal"] = round(ms["imu"] + ms["wlocal_recorded_pose"], 4)
res["launches"]["imu_plus_wlocal"] = res["launches"]["imu"] + res["launches"]["wlocal_recorded_pose"]
res["finetune_minus_sum_ms"] = round(ms["wlocal_finetune_imu"] - ms["imu_plus_wlocal"], 4)
res["finetune_minus_sum_rel"] = round(res["finetune_minus_sum_ms"] / ms["imu_plus_wlocal"], 5)
parts = collections.Counter(res["entry_points"]["imu"]) + collections.Counter(res["entry_points"]["wlocal_recorded_pose"])
fine = res["entry_points"]["wlocal_finetune_imu"]
res["launch_difference"] = {k: fine.get(k, 0) - parts.get(k, 0) for k in sorted(set(parts) | set(fine)) if fine.get(k, 0) != parts.get(k, 0)}
print("wlocal_finetune_imu %.3f ms against imu + wlocal_recorded_pose %.3f ms: %+.3f ms (%+.2f %%); launches %d against %d; by entry point: %s"
      % (ms["wlocal_finetune_imu"], ms["imu_plus_wlocal"], res["finetune_minus_sum_ms"], 100 * res["finetune_minus_sum_rel"],
         res["launches"]["wlocal_finetune_imu"], res["launches"]["imu_plus_wlocal"], res["launch_difference"]))
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
