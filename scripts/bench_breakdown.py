"""What the error breakdown (evaluate_full / dense_infer under breakdown=(bin_cm, nbins): --infer [--dense] --breakdown) costs, in ONE
process:

  python scripts/bench_breakdown.py OUT.json

(a) device-event time of the new launches alone on a table of 32 768 rows of 43 columns (mmego_pose_errors' width; values like joint
    errors in metres): mmego_colsum_groups with G = 13 and G = 256, the ids sorted by group (what --infer and dense rows are) and
    shuffled; mmego_hist_groups with 4096 bins of 0.05 cm over the 21 joint columns -- pooled without ids, pooled by 13 groups, per
    column; beside them, as the yardstick, mmego_colsum on the same table -- the forms alternating, 20 chains of 10 calls after 3, a
    chain per event pair so that the timed window is not a single launch;
(b) the dense pass, wall clock to its last host read, on Sample_data-shaped synthetic frames (scripts/bench_frame_store.py's generator:
    223 recordings, 19 706 frames, dealt here to 13 actions; frame_no 20, window minibatch 64) at stride 5: without the argument
    and with breakdown=evaluation.BREAKDOWN_BINS -- alternating, five rounds, medians, and the band of the rounds."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_dense_bones import chains_us, golden, load  # noqa: E402
from bench_frame_store import rounds, synthetic_frames  # noqa: E402
from mmego_amd import dense, evaluation, hip, nets, ops, processors  # noqa: E402
from mmego_amd.config import ConfigDemo  # noqa: E402
from mmego_amd.data import PosePC  # noqa: E402

dev = torch.device("cuda:0")
T, B, ROWS, C = 20, 64, 32768, 43


def main(path):
    hip.lib()
    ConfigDemo.gt_head_pose = True
    base = processors._Base(ConfigDemo, make_dirs=False)
    up, lo = load(nets.UpperNet(), golden("w_upper_pretrained.npz")), load(nets.LowerNet(64), golden("w_lower_pretrained.npz"))
    bin_cm, nbins = evaluation.BREAKDOWN_BINS
    res = {"shape": {"rows": ROWS, "columns": C, "bin_cm": bin_cm, "nbins": nbins, "frame_no": T, "window_minibatch": B},
           "method": "launches: device events around a chain of 10 calls, the forms alternating, 20 repetitions after 3, per call; passes: "
                     "wall clock around a whole pass (its last statement is a device -> host read), one warm pass each, then the passes "
                     "alternating, five rounds, medians"}

    # (a) the launches
    rng = np.random.default_rng(0)
    X = torch.as_tensor(rng.gamma(2.0, 0.03, (ROWS, C)).astype(np.float32)).to(dev)
    out1 = torch.empty(C, device=dev)
    forms = {"colsum (the yardstick)": lambda: ops.colsum(X, out1)}
    keep = []
    for G in (13, 256):
        for order in ("sorted", "shuffled"):
            ids = np.sort(rng.integers(0, G, ROWS)) if order == "sorted" else rng.integers(0, G, ROWS)
            ids = torch.as_tensor(ids.astype(np.int32)).to(dev)
            out, count = torch.empty((G, C), device=dev), torch.empty(G, device=dev)
            keep.append((ids, out, count))
            forms["colsum_groups G = %d, %s" % (G, order)] = (lambda ids=ids, G=G, out=out, count=count:
                                                              hip.call("colsum_groups", X, C, ROWS, C, ids, G, out, C, count))
    ids13 = keep[0][0]
    inv = 100.0 / bin_cm
    h1, l1 = torch.empty((1, nbins), dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    h13, l13 = torch.empty((13, nbins), dtype=torch.int32, device=dev), torch.empty(13, dtype=torch.int32, device=dev)
    hj, lj = torch.empty((1, 21, nbins), dtype=torch.int32, device=dev), torch.empty((1, 21), dtype=torch.int32, device=dev)
    forms["hist_groups pooled, no ids (21 columns)"] = lambda: hip.call("hist_groups", X, C, ROWS, 21, None, 1, inv, nbins, 1, h1, l1)
    forms["hist_groups pooled, G = 13 (21 columns)"] = lambda: hip.call("hist_groups", X, C, ROWS, 21, ids13, 13, inv, nbins, 1, h13, l13)
    forms["hist_groups per column, no ids (21 columns)"] = lambda: hip.call("hist_groups", X, C, ROWS, 21, None, 1, inv, nbins, 0, hj, lj)
    t = chains_us(forms)
    for k in list(t):
        if k.startswith("colsum_groups"):
            t[k + " / colsum"] = round(t[k]["median"] / t["colsum (the yardstick)"]["median"], 2)
    assert int(h1.sum()) + int(l1.sum()) == ROWS * 21 and torch.equal(hj.sum(dim=1), h1)
    res["launch_us"] = t
    print("launch_us", t)

    # (b) the pass
    dec = synthetic_frames()
    PosePC._decode = lambda self: dec
    np.random.seed(0)
    ds = PosePC(train=False, vis=True, batch_length=T, root=os.path.join(ROOT, "scripts"), keep_frames=True)
    n_rec = len(dec["snip_len"])
    ds.rec_action_, ds.rec_snippet_ = (np.arange(n_rec) * 13 // n_rec + 1).astype(np.int64), np.arange(n_rec, dtype=np.int64)      # 13 actions
    res["frames"], res["recordings"], res["actions"] = int(len(ds.frame_npts_)), n_rec, 13

    def timed_pass(**more):
        def s():
            t0 = time.perf_counter()
            dense.dense_infer(base, None, up, lo, ds, 5, batch_size=B, **more)
            return time.perf_counter() - t0
        return s
    timers = {"stride 5": timed_pass(), "stride 5, breakdown": timed_pass(breakdown=evaluation.BREAKDOWN_BINS)}
    for f in timers.values():
        f()
    res["pass_s"] = rounds(timers, 5)
    base_s = res["pass_s"]["stride 5"]
    res["pass_s"]["band of the plain rounds / median"] = round((max(base_s["rounds"]) - min(base_s["rounds"])) / base_s["median"], 4)
    res["pass_s"]["breakdown / plain"] = round(res["pass_s"]["stride 5, breakdown"]["median"] / base_s["median"], 4)
    print("pass_s", res["pass_s"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "breakdown.json")
