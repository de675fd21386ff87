"""What the floor option of dense inference (dense.dense_infer(floor=(mode, contact_cm, margin_cm)): --infer --dense --floor M) costs,
in ONE process:

  python scripts/bench_dense_floor.py OUT.json

(a) device-event time of the two launches alone, mmego_floor_stats and mmego_floor_clamp (out of place, with lifted and fallback), at
    512 and 32 768 rows of random standing legs (tests/floor_ref.py's draw: about a third of the legs reach under their plane) -- the
    forms alternating, 20 chains of 10 calls after 3, a chain per event pair so that the timed window is not a single launch;
(b) the dense pass, wall clock to its last host read, on Sample_data-shaped synthetic frames (scripts/bench_frame_store.py's generator:
    223 recordings, about 19 100 frames; frame_no 20, window minibatch 64) at stride 5: without the argument (the launches of the pass
    before this option), with floor=("measure", 6, 0) and with floor=("clamp", 6, 0) -- alternating, five rounds, medians, and the band
    of the rounds.  The synthetic frames get the plane z = 0.2, the median height of their random joints, and random flags.
No bar is set: the figures are a record against the same pass without the argument."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import floor_ref as fref  # noqa: E402
from bench_dense_bones import chains_us, golden, load  # noqa: E402
from bench_frame_store import rounds, synthetic_frames  # noqa: E402
from mmego_amd import dense, hip, nets, ops, processors  # noqa: E402
from mmego_amd.config import ConfigDemo  # noqa: E402
from mmego_amd.data import PosePC  # noqa: E402

dev = torch.device("cuda:0")
T, B = 20, 64


def main(path):
    hip.lib()
    ConfigDemo.gt_head_pose = True
    base = processors._Base(ConfigDemo, make_dirs=False)
    up, lo = load(nets.UpperNet(), golden("w_upper_pretrained.npz")), load(nets.LowerNet(64), golden("w_lower_pretrained.npz"))
    res = {"shape": {"frame_no": T, "window_minibatch": B},
           "method": "launches: device events around a chain of 10 calls, the forms alternating, 20 repetitions after 3, per call; passes: "
                     "wall clock around a whole pass (its last statement is a device -> host read), one warm pass each, then the passes "
                     "alternating, five rounds, medians"}

    # (a) the launches
    forms, keep = {}, []
    for rows in (512, 32768):
        rng = np.random.default_rng(rows)
        legs, ground = fref.random_legs(rng, rows)
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        src, gr, tgt = f32(legs), f32(ground), f32(rng.normal(0.0, 0.5, (rows, 63)))
        contact, seg = f32(rng.integers(0, 2, (rows, 2))), torch.zeros(rows, dtype=torch.int32, device=dev)
        out, dst = torch.empty((rows, ops.FLOOR_W), device=dev), torch.empty((rows, 24), device=dev)
        lifted, fell = torch.empty(rows, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
        ops.floor_stats(src, tgt, gr, contact, seg, 0.06, out)         # (the host checks, once)
        ops.floor_clamp(src, gr, seg, 0.0, dst, lifted, fell)
        keep.append((src, gr, tgt, contact, seg, out, dst, lifted, fell))

        def add(rows=rows, t=keep[-1]):
            src, gr, tgt, contact, seg, out, dst, lifted, fell = t
            forms["floor_stats, %d rows" % rows] = lambda: hip.call("floor_stats", src, 24, tgt, 63, gr, contact, seg, rows, 0.06, out)
            forms["floor_clamp, %d rows" % rows] = lambda: hip.call("floor_clamp", src, 24, gr, seg, rows, 0.0, dst, 24, lifted, fell)
        add()
        res.setdefault("lifted_rows", {})[str(rows)] = int((lifted > 0).sum())
    res["launch_us"] = chains_us(forms)
    print("launch_us", res["launch_us"])

    # (b) the pass
    dec = synthetic_frames()
    PosePC._decode = lambda self: dec
    np.random.seed(0)
    ds = PosePC(train=False, vis=True, batch_length=T, root=os.path.join(ROOT, "scripts"), keep_frames=True)
    F = len(ds.frame_npts_)
    ds.frame_ground_ = np.tile(np.float32([0.0, 0.0, 1.0, -0.2]), (F, 1))
    ds.frame_contact_ = np.random.default_rng(1).integers(0, 2, (F, 2)).astype(np.uint8)
    res["frames"] = int(F)

    def timed_pass(**more):
        def s():
            t0 = time.perf_counter()
            dense.dense_infer(base, None, up, lo, ds, 5, batch_size=B, **more)
            return time.perf_counter() - t0
        return s
    timers = {"stride 5, no argument": timed_pass(), "stride 5, floor measure": timed_pass(floor=("measure", 6, 0)),
              "stride 5, floor clamp": timed_pass(floor=("clamp", 6, 0))}
    for t in timers.values():
        t()
    res["pass_s"] = rounds(timers, 5)
    base_s = res["pass_s"]["stride 5, no argument"]
    res["pass_s"]["band of the no-argument rounds / median"] = round((max(base_s["rounds"]) - min(base_s["rounds"])) / base_s["median"], 4)
    for k in ("measure", "clamp"):
        res["pass_s"]["floor %s / no argument" % k] = round(res["pass_s"]["stride 5, floor %s" % k]["median"] / base_s["median"], 4)
    print("pass_s", res["pass_s"])
    s, _ = dense.dense_infer(base, None, up, lo, ds, 5, batch_size=B, floor=("clamp", 6, 0))
    res["clamp_synthetic"] = {"note": "pretrained weights on random clouds against random targets: the figures show the mechanics, not accuracy",
                              **{k: s[k] for k in ("covered_frames", "lifted_frames", "lift_cm", "floor_fallback", "penetration_rate",
                                                   "unclamped_penetration_rate", "unclamped_penetration_cm", "all_cm", "unclamped_all_cm")}}
    print("clamp_synthetic", res["clamp_synthetic"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "dense_floor.json")
