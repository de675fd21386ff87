"""Cost of a --finetune_imu step (Upper_Net + IMU_Net trained end to end) at the bench batch B=64, T=8, N=128, HIP-graph replay,
beside its two halves measured in the same run: the stage-1 step (train_step.ImuStep) and the Upper stage's step with the recorded
head pose (train_step.StageStep, no IMU_Net).  Then the per-entry-point split of one eager fine-tuning body (event-timed), which
shows what the head-pose gradient kernels add.

  python scripts/bench_finetune_step.py [--out profiles/finetune_step.json] [--replay-only]

--replay-only: just 20 replays of the fine-tuning step (the program to put behind `rocprofv3 --kernel-trace --stats --`)."""
import collections
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets  # noqa: E402
from mmego_amd.train_step import ImuStep, StageStep  # noqa: E402

NEW = ("transform2h_backward", "head_fk_loss_pose", "head_fk_backward_pose")

dev = torch.device("cuda:0")
hip.lib()
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


def make(kind):
    torch.manual_seed(1)
    himu = nets.IMUNet(15, 9, 512, 2, True, 0).to(dev).train()
    hup = nets.UpperNet().to(dev).train()
    if kind == "stage1":
        st = ImuStep(himu, lr=1e-4, use_graph=True)
        st.bind(imu, Rg, target)
    elif kind == "upper_recorded_pose":
        st = StageStep("upper", hup, None, lr=3e-5, use_graph=True)
        st.bind(x, imu, body, target, R_gt=Rg)
    elif kind == "upper_frozen_imu":
        st = StageStep("upper", hup, himu.eval(), lr=3e-5, use_graph=True)
        st.bind(x, imu, body, target)
    else:
        st = StageStep("upper", hup, himu, lr=3e-5, use_graph=kind == "finetune", finetune_imu=True, imu_lr=3e-5)
        st.bind(x, imu, body, target)
    return st


if "--replay-only" in sys.argv:
    st = make("finetune")
    print("finetune step: %.3f ms" % timed(st.step, n=20))
    sys.exit(0)

res = {"shape": {"B": B, "T": T, "N": N}, "method": "HIP-graph replay + fused Adam launches, 50 steps after 5, wall clock / step",
       "ms_per_step": {}}
for kind in ("stage1", "upper_recorded_pose", "upper_frozen_imu", "finetune"):
    st = make(kind)
    res["ms_per_step"][kind] = round(timed(st.step), 4)
    print("%-22s %.3f ms per step" % (kind, res["ms_per_step"][kind]))
    del st
res["ms_per_step"]["stage1_plus_upper"] = round(res["ms_per_step"]["stage1"] + res["ms_per_step"]["upper_recorded_pose"], 4)

# per entry point: one eager body, every launch between two events
st = make("finetune_eager")
for _ in range(3):
    st.step()
torch.cuda.synchronize()
rec = collections.defaultdict(list)
orig = hip._launch


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
tot = {k: (sum(a.elapsed_time(b) for a, b in v), len(v)) for k, v in rec.items()}
body_ms = sum(ms for ms, _ in tot.values())
res["eager_body_event_ms"] = round(body_ms, 4)
res["new_entry_points"] = {k: {"launches": tot[k][1], "ms": round(tot[k][0], 5), "share_of_body": round(tot[k][0] / body_ms, 6)}
                           for k in NEW if k in tot}
for k, (ms, cnt) in sorted(tot.items(), key=lambda kv: -kv[1][0])[:12]:
    print("   %-28s %4d launches %8.3f ms" % (k, cnt, ms))
for k, v in res["new_entry_points"].items():
    print("   new: %-24s %s" % (k, v))
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
