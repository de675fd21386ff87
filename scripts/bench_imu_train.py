"""Stage-1 (IMU_Net) training step on the HIP path: ms per step at the reference's batch (B=20 sequences x T=20 frames x 20
samples) and at the bench batch (B=64, T=8), plus the per-entry-point split of one step.

  python scripts/bench_imu_train.py [--dropout P] [--ab OUT.json]

--dropout P: the net is built with nn.LSTM(dropout=P) between its BiLSTM layers (default 0).
--ab OUT.json: what inter-layer dropout costs, in ONE process: at B=64, T=8 the graph-replayed stage-1 step (train_step.ImuStep) and the
--finetune_imu step (train_step.StageStep, N=128) with rate 0 and rate P (default 0.1) alternating, three rounds, medians; and the
mmego_lstm_dropout launch on rnn_fast's 10 240 x 1024 layer output beside ops.copy2d of the same tensor."""
import os
import sys
import time
import collections

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmego_amd import hip, imu_train, nets  # noqa: E402
from mmego_amd.params import FusedAdam  # noqa: E402

dev = torch.device("cuda:0")
hip.lib()
P_DROP = float(sys.argv[sys.argv.index("--dropout") + 1]) if "--dropout" in sys.argv else 0.0


def ab(path, p):
    import json
    import statistics
    from mmego_amd import ops
    from mmego_amd.train_step import ImuStep, StageStep
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

    def make(kind, rate):
        torch.manual_seed(1)
        himu = nets.IMUNet(15, 9, 512, 2, True, rate).to(dev).train()
        if kind == "stage1":
            st = ImuStep(himu, lr=1e-4, use_graph=True)
            st.bind(imu, Rg, target)
        else:
            st = StageStep("upper", nets.UpperNet().to(dev).train(), himu, lr=3e-5, use_graph=True, finetune_imu=True, imu_lr=3e-5)
            st.bind(x, imu, body, target)
        return st
    res = {"shape": {"B": B, "T": T, "N": N}, "p": p,
           "method": "HIP-graph replay + fused Adam launches, 50 steps after 5, wall clock / step; rate 0 and rate p alternate in one "
                     "process, three rounds each", "ms_per_step": {}}
    for kind in ("stage1", "finetune"):
        steps = {rate: make(kind, rate) for rate in (0.0, p)}
        runs = {rate: [] for rate in steps}
        for _ in range(3):
            for rate, st in steps.items():
                runs[rate].append(round(timed(st.step), 4))
        res["ms_per_step"][kind] = {"p=%g" % rate: {"rounds": v, "median": statistics.median(v)} for rate, v in runs.items()}
        print(kind, res["ms_per_step"][kind])
        del steps
    # the launch itself beside the project's streaming yardstick, on rnn_fast's layer output (84 MB in and out), event-timed
    rows, cols = B * T * 20, 1024
    src, dst = torch.randn(rows, cols, device=dev), torch.empty(rows, cols, device=dev)
    word = torch.tensor([12345], dtype=torch.int64, device=dev)

    def launch_us(fn, n=20):
        for _ in range(3):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return round(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3, 2)
    res["launch_us"] = {"rows": rows, "cols": cols, "bytes_moved": 8 * rows * cols,
                        "lstm_dropout": launch_us(lambda: ops.lstm_dropout(src, dst, p, word, 0)),
                        "lstm_dropout_in_place": launch_us(lambda: ops.lstm_dropout(dst, dst, p, word, 0)),
                        "copy2d": launch_us(lambda: ops.copy2d(src, dst)),
                        "torch_copy": launch_us(lambda: dst.copy_(src))}
    small = torch.randn(B * T, cols, device=dev)
    res["launch_us"]["lstm_dropout_512x1024"] = launch_us(lambda: ops.lstm_dropout(small, small, p, word, 8))
    for k in ("lstm_dropout", "lstm_dropout_in_place", "copy2d", "torch_copy"):
        res["launch_us"][k + "_TBps"] = round(8 * rows * cols / res["launch_us"][k] / 1e6, 3)
    print(res["launch_us"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)


if "--ab" in sys.argv:
    ab(sys.argv[sys.argv.index("--ab") + 1], P_DROP if P_DROP > 0 else 0.1)
    sys.exit(0)

torch.manual_seed(0)
net = nets.IMUNet(15, 9, 512, 2, True, P_DROP).to(dev).train()
opt = FusedAdam(net.flat(), lr=1e-4, weight_decay=0.001)
loss = torch.zeros(1, device=dev)
for B, T in ((20, 20), (64, 8)):
    imu = torch.randn(B, T, 20, 15, device=dev)
    Rg = torch.linalg.qr(torch.randn(B, T, 3, 3, device=dev))[0].contiguous()
    head = torch.randn(B, T, 3, device=dev)

    def step():
        with torch.no_grad():
            R, t = imu_train.forward_train(net, imu)
            dR, dt = torch.empty_like(R), torch.empty_like(t)
            hip.call("imu_loss", R.contiguous(), t.contiguous(), Rg, head, B * T, 1.0, loss, dR, dt)
            imu_train.backward(net, dR, dt)
        opt.step()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 10
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    print("B=%d T=%d: %.2f ms per stage-1 step (eager)" % (B, T, (time.perf_counter() - t0) / n * 1e3))
    from mmego_amd.train_step import ImuStep
    st = ImuStep(net, lr=1e-4, use_graph=True)
    st.opt = opt
    tgt = torch.zeros(B, T, 21, 3, device=dev)
    tgt[:, :, 20] = head
    st.bind(imu, Rg, tgt)
    for _ in range(3):
        st.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        st.step()
    torch.cuda.synchronize()
    print("B=%d T=%d: %.2f ms per stage-1 step (HIP graph)" % (B, T, (time.perf_counter() - t0) / 20 * 1e3))
    # per entry point
    rec = collections.defaultdict(list)
    orig = hip.call

    def timed(name, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); orig(name, *a); e1.record()
        key = name
        if name == "gemm":      # (A, sam, sak, B, sbk, sbn, C, scm, scn, bias, M, N, K, nbatch, ..., nsplit)
            key = "gemm M%d N%d K%d %s%s split%d" % (a[10], a[11], a[12], "k" if a[2] == 1 else "m", "k" if a[4] == 1 else "n", a[20])
        rec[key].append((e0, e1))
    hip.call = timed
    step()
    torch.cuda.synchronize()
    hip.call = orig
    tot = {k: (sum(a.elapsed_time(b) for a, b in v), len(v)) for k, v in rec.items()}
    for k, (ms, cnt) in sorted(tot.items(), key=lambda kv: -kv[1][0])[:14]:
        print("   %-40s %4d launches %8.3f ms  (%.1f us each)" % (k, cnt, ms, ms / cnt * 1e3))
