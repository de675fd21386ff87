"""Cost of a --finetune_upper step (Lower_Net + Upper_Net trained jointly, stage 3) at the bench batch B=64, T=8, N=128, recorded head
pose, HIP-graph replay, beside the two steps it is made of, measured in the same run: the Upper stage's step and the plain Lower stage's
step (train_step.StageStep).  The joint body is those two bodies minus one eval-mode Upper_Net forward plus a handful of small launches,
so the bar is: joint <= upper + lower.  Then the per-entry-point split of one eager joint body (event-timed), which shows what the
input-gradient kernels add.

  python scripts/bench_finetune_upper_step.py [--out profiles/finetune_upper_step.json] [--replay-only]

--replay-only: just 20 replays of the joint step (the program to put behind `rocprofv3 --kernel-trace --stats --`)."""
import collections
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, nets  # noqa: E402
from mmego_amd.train_step import StageStep  # noqa: E402

NEW = ("lower_inputs_backward", "bn_input_grad")

dev = torch.device("cuda:0")
hip.lib()
B, T, N = 64, 8, 128
g = torch.Generator().manual_seed(0)
x = torch.randn(B, T, N, 6, generator=g).to(dev)
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
    hup = nets.UpperNet().to(dev).train()
    hlo = nets.LowerNet(64).to(dev).train()
    if kind == "upper":
        st = StageStep("upper", hup, None, lr=3e-5, use_graph=True)
    elif kind == "lower":
        st = StageStep("lower", hlo, None, upper_frozen=hup.eval(), lr=3e-5, use_graph=True)
    else:
        st = StageStep("lower", hlo, None, upper_frozen=hup, lr=3e-5, use_graph=kind == "joint", finetune_upper=True, upper_lr=3e-5)
    st.bind(x, None, body, target, R_gt=Rg)
    return st


if "--replay-only" in sys.argv:
    st = make("joint")
    print("joint step: %.3f ms" % timed(st.step, n=20))
    sys.exit(0)

res = {"shape": {"B": B, "T": T, "N": N}, "method": "HIP-graph replay + fused Adam launches, 300 steps after 5, wall clock / step; three "
       "interleaved rounds, the median per kind", "ms_per_step": {}, "rounds": {}}
steps = {kind: make(kind) for kind in ("upper", "lower", "joint")}
for kind, st in steps.items():
    timed(st.step, n=5)                                    # (capture + first replays)
for kind in steps:
    res["rounds"][kind] = []
for _ in range(3):                                         # interleaved rounds: a drift of the clocks hits every kind alike
    for kind, st in steps.items():
        res["rounds"][kind].append(round(timed(st.step, n=300), 4))
for kind in steps:
    res["ms_per_step"][kind] = sorted(res["rounds"][kind])[1]
    print("%-8s %.3f ms per step  (rounds: %s)" % (kind, res["ms_per_step"][kind], res["rounds"][kind]))
res["ms_per_step"]["upper_plus_lower"] = round(res["ms_per_step"]["upper"] + res["ms_per_step"]["lower"], 4)
res["joint_within_bar"] = bool(res["ms_per_step"]["joint"] <= res["ms_per_step"]["upper_plus_lower"])
print("joint %.3f ms against upper + lower %.3f ms: %s" % (res["ms_per_step"]["joint"], res["ms_per_step"]["upper_plus_lower"],
                                                           "inside the bar" if res["joint_within_bar"] else "OUTSIDE the bar"))
del steps

# per entry point: one eager body, every launch between two events
st = make("joint_eager")
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
res["eager_body_launches"] = sum(cnt for _, cnt in tot.values())
res["entry_points"] = {k: {"launches": cnt, "ms": round(ms, 5)} for k, (ms, cnt) in sorted(tot.items(), key=lambda kv: -kv[1][0])}
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
