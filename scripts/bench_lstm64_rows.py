"""The two forms of the BiLSTM(64) recurrence kernels (MMEGO_LSTM64_ROWS = 4 | 16, csrc/lstm.hip) side by side: forward (stashes on) and
backward launches over batch sizes and two sequence lengths, 40 launches of a kind captured in one HIP graph, replays timed with events,
the forms alternating, median of the rounds.  us per launch, us per step from the two lengths ((t(2T) - t(T)) / T), and which form the
launchers choose by themselves at each batch size.

usage: python scripts/bench_lstm64_rows.py [out.json]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mmego_amd import hip  # noqa: E402

ENV, N, ROUNDS, REPLAYS = "MMEGO_LSTM64_ROWS", 40, 5, 20
dev = torch.device("cuda:0")


def graphs(B, T):
    """-> {(kind, rows): captured graph of N launches}; the form is chosen when a launch is captured."""
    g = torch.Generator(device="cpu").manual_seed(B * 100 + T)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.1).to(dev)
    xp, w, b = torch.randn(B * T, 512, generator=g).to(dev), [r(256, 64) for _ in range(2)], [r(256) for _ in range(2)]
    out, hn, cn = torch.empty(B * T, 128, device=dev), torch.empty(2, B, 64, device=dev), torch.empty(2, B, 64, device=dev)
    gates, cst, hp = torch.empty(2, T, B, 256, device=dev), torch.empty(2, T, B, 64, device=dev), torch.empty(2, B * T, 64, device=dev)
    dout, dg = torch.randn(B * T, 128, generator=g).to(dev), torch.empty(B * T, 512, device=dev)
    fwd = lambda: hip.call("lstm64_forward", B, T, xp, xp[:, 256:], 512, w[0], w[1], b[0], b[1], None, None, None, None, out, 128, hn[0], hn[1],
                           cn[0], cn[1], gates[0], gates[1], cst[0], cst[1], hp[0], hp[1], None, None, 0.0, None, 0)
    bwd = lambda: hip.call("lstm64_backward", B, T, dout, 128, gates[0], gates[1], cst[0], cst[1], None, None, w[0], w[1], dg, dg[:, 256:], 512)
    res, keep = {}, (xp, w, b, out, hn, cn, gates, cst, hp, dout, dg)
    for rows in (4, 16):
        os.environ[ENV] = str(rows)
        for kind, fn in (("fwd", fwd), ("bwd", bwd)):
            fn()
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            with torch.cuda.stream(s), torch.cuda.graph(cg, stream=s):
                for _ in range(N):
                    fn()
            res[(kind, rows)] = cg
    del os.environ[ENV]
    return res, keep


def timed(cg):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cg.replay()
    e0.record()
    for _ in range(REPLAYS):
        cg.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPLAYS * N)


def main():
    res = {"what": "us per launch (HIP-graph replay of %d launches, median of %d alternating rounds), B x T, forward with stashes / backward" % (N, ROUNDS),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "shapes": []}
    T = 8
    for B in (16, 64, 128, 256, 384, 496, 512, 768, 1024, 2048):
        row = {"B": B, "launcher_takes_rows": hip.lib().mmego_lstm64_rows(B)}
        us = {}
        for TT in (T, 2 * T):
            gs, keep = graphs(B, TT)
            samples = {k: [] for k in gs}
            for _ in range(ROUNDS):
                for k, cg in gs.items():
                    samples[k].append(timed(cg))
            for (kind, rows), v in samples.items():
                us[(kind, rows, TT)] = statistics.median(v)
            del gs, keep
        for kind in ("fwd", "bwd"):
            for rows in (4, 16):
                row["%s_rows%d" % (kind, rows)] = {"us_T%d" % T: round(us[(kind, rows, T)], 2), "us_T%d" % (2 * T): round(us[(kind, rows, 2 * T)], 2),
                                                   "us_per_step": round((us[(kind, rows, 2 * T)] - us[(kind, rows, T)]) / T, 3)}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
