"""What the renderer of dense inference (dense.dense_infer(render=...): --infer --dense --render DIR) costs.  Four steps:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o render -- python scripts/bench_render.py trace
  python scripts/bench_render.py host HOST.json [PICTURE.png]
  python scripts/bench_render.py parts PARTS.json
  python scripts/bench_render.py summary DIR HOST.json PARTS.json profiles/render.json

trace   the program behind rocprofv3, a run of its own: 256 frames of a swaying standing skeleton with N = 128 radar returns each, one
        256 x 256 view -- ops.render_prims and ops.render_raster 20 times after 3, and ops.fill 20 times over as many BYTES as the
        raster writes (256 x 256 x 256 x 3), the floor for a kernel whose product is its store traffic.
host    wall clock (every timed piece ends in a device -> host read or on the host): render.render_frames of a 256-frame recording at
        256 px (two views), its device -> host copy, render.write_apng of it; and the dense pass on the test tree of
        tests/test_dense_infer_gpu.py (91 frames, stride 5) without and with render at 256 px -- alternating, five rounds, medians.
parts   where the raster's time goes, by device events (chains of 10 calls, 20 repetitions, the forms alternating): the same launch with
        P = 0 (the stores alone), with the 262 primitives of every frame moved off the image (the table read and the cull, no survivor),
        with the N = 0 scene (134 primitives) and with the whole scene; and the mean number of survivors per tile, counted on the host.
summary the three kernels' rows of rocprofv3's kernel statistics and the host figures, as one JSON.
No bar is set: the parent of this option cannot draw at all."""
import csv
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F, N, SIZE = 256, 128, 256
# a standing skeleton in metres, z up, the floor z = 0: the 21 joints in the loader's order
POSE = np.array([[0, 0, .95], [0, 0, 1.15], [0, 0, 1.4], [0, 0, 1.5], [.18, 0, 1.42], [.25, 0, 1.15], [.27, 0, .9], [.27, 0, .82], [-.18, 0, 1.42],
                 [-.25, 0, 1.15], [-.27, 0, .9], [-.27, 0, .82], [.1, 0, .92], [.11, 0, .5], [.11, 0, .08], [.11, .12, .02], [-.1, 0, .92],
                 [-.11, 0, .5], [-.11, 0, .08], [-.11, .12, .02], [0, 0, 1.65]])


def scene(frames=F, n=N, seed=0):
    """Host arrays of a swaying standing skeleton: pred, tgt [frames, 63], ground [frames, 4], cloud [frames, n, 6], seg [frames]."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[:, None, None] / 10.0
    tgt = POSE[None] + 0.05 * np.sin(t + POSE[None, :, 2:3] * 3.0) * np.array([1.0, 0.6, 0.0]) * POSE[None, :, 2:3]
    pred = tgt + rng.normal(0, 0.03, tgt.shape)
    at = tgt[np.arange(frames)[:, None], rng.integers(0, 21, (frames, n))] + rng.normal(0, 0.1, (frames, n, 3))
    cloud = np.concatenate([at, np.linalg.norm(at, axis=2, keepdims=True), rng.normal(0, 0.5, (frames, n, 1)), rng.uniform(10, 46, (frames, n, 1))], 2)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(pred=f32(pred.reshape(frames, 63)), tgt=f32(tgt.reshape(frames, 63)), ground=f32(np.tile([0.0, 0.0, 1.0, 0.0], (frames, 1))),
                cloud=f32(cloud), seg=np.zeros(frames, dtype=np.int32))


def on_device(c, dev):
    import torch
    return {k: torch.as_tensor(v).to(dev) for k, v in c.items()}


def trace():
    import torch
    from mmego_amd import ops, render
    dev = torch.device("cuda:0")
    c = scene()
    d = on_device(c, dev)
    cam = torch.as_tensor(render.camera(c["tgt"], c["ground"], "front", SIZE)).to(dev)
    prims = torch.empty((F, ops.RENDER_FIXED + N, ops.RENDER_REC), device=dev)
    out = torch.empty((F, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    same_bytes = torch.empty(out.numel() // 4, device=dev)
    for _ in range(23):
        ops.render_prims(d["pred"], d["tgt"], d["ground"], d["cloud"], d["seg"], cam, 1.0, prims)
        ops.render_raster(prims, out)
        ops.fill(same_bytes, 1.0)
    torch.cuda.synchronize()
    print("trace: %d frames, N = %d, %d px, %d output bytes" % (F, N, SIZE, out.numel()))


def median_of(fn, rounds=5):
    fn()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ts.append(round(time.perf_counter() - t0, 4))
    return {"rounds": ts, "median": float(np.median(ts))}


def host(path, picture=None):
    import torch
    import test_dense_infer_gpu as di
    from mmego_amd import dense, nets, processors, render
    from mmego_amd.config import ConfigDemo
    from mmego_amd.data import PosePC
    dev = torch.device("cuda:0")
    d = on_device(scene(), dev)
    res = {"shape": {"frames": F, "N": N, "size_px": SIZE, "frame_bytes": SIZE * 2 * SIZE * 3},
           "method": "wall clock, one warm call, then five rounds, medians; every timed piece ends in a device -> host read or on the host"}
    draw = lambda: render.render_frames(d["pred"], d["tgt"], d["ground"], d["cloud"], d["seg"], SIZE)
    img = draw()
    res["render_frames_and_copy_s"] = median_of(lambda: draw().cpu())
    res["copy_only_s"] = median_of(lambda: img.cpu())
    frames = img.cpu().numpy()
    tmp = tempfile.mkdtemp(prefix="bench_render_")
    res["write_apng_s"] = median_of(lambda: render.write_apng(os.path.join(tmp, "a.png"), frames, 10))
    res["apng_bytes"] = os.path.getsize(os.path.join(tmp, "a.png"))
    if picture:
        render.write_apng(picture, frames[:40], 10)
    # the dense pass on the test tree
    data = os.path.join(tmp, "Sample_data")
    di._make_dataset(data, np.random.default_rng(0))
    np.random.seed(3)
    ds = PosePC(train=False, vis=True, keep_frames=True, batch_length=di.T, root=data)
    ConfigDemo.gt_head_pose = True
    base = processors._Base(ConfigDemo, make_dirs=False)
    torch.manual_seed(0)
    up, lo = nets.UpperNet().to(dev).eval(), nets.LowerNet(64).to(dev).eval()
    plain = lambda: dense.dense_infer(base, None, up, lo, ds, 5, batch_size=4)
    drawn = lambda: dense.dense_infer(base, None, up, lo, ds, 5, batch_size=4, render=(os.path.join(tmp, "pictures"), SIZE, None, 10))
    plain(), drawn()
    rounds = {"without render": [], "with render, 256 px": []}
    for _ in range(5):
        for name, fn in (("without render", plain), ("with render, 256 px", drawn)):
            t0 = time.perf_counter()
            fn()
            rounds[name].append(round(time.perf_counter() - t0, 4))
    res["dense_pass_test_tree_s"] = {k: {"rounds": v, "median": float(np.median(v))} for k, v in rounds.items()}
    res["dense_pass_test_tree_s"]["frames"], res["dense_pass_test_tree_s"]["rendered_frames"] = di.F, 84
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


def parts(path):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from bench_dense_bones import chains_us
    from mmego_amd import ops, render
    dev = torch.device("cuda:0")
    c = scene()
    d = on_device(c, dev)
    cam = torch.as_tensor(render.camera(c["tgt"], c["ground"], "front", SIZE)).to(dev)
    prims = ops.render_prims(d["pred"], d["tgt"], d["ground"], d["cloud"], d["seg"], cam, 1.0, torch.empty((F, 134 + N, 12), device=dev))
    bare = ops.render_prims(d["pred"], d["tgt"], d["ground"], d["cloud"][:, :0].contiguous(), d["seg"], cam, 1.0, torch.empty((F, 134, 12), device=dev))
    away = prims.clone()
    away[:, :, :4] += 10000.0
    none = torch.empty((F, 0, 12), device=dev)
    out = torch.empty((F, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    forms = {"P = 0 (stores alone)": lambda: ops.render_raster(none, out), "262 primitives, all culled": lambda: ops.render_raster(away, out),
             "134 primitives (N = 0)": lambda: ops.render_raster(bare, out), "262 primitives (N = 128)": lambda: ops.render_raster(prims, out)}
    res = {"raster_us": chains_us(forms)}
    # survivors per 32 x 32 tile, as the kernel culls: the segment's box grown by r + 0.5 against the tile's pixel centres
    p = prims.cpu().numpy().astype(np.float64)
    R = p[:, :, 4] + 0.5
    ok = (p[:, :, 5] > 0)
    lo_x, hi_x = np.minimum(p[:, :, 0], p[:, :, 2]) - R, np.maximum(p[:, :, 0], p[:, :, 2]) + R
    lo_y, hi_y = np.minimum(p[:, :, 1], p[:, :, 3]) - R, np.maximum(p[:, :, 1], p[:, :, 3]) + R
    counts = []
    for ty in range(SIZE // 32):
        for tx in range(SIZE // 32):
            x0, y0 = 32 * tx + 0.5, 32 * ty + 0.5
            counts.append((ok & (lo_x <= x0 + 31) & (hi_x >= x0) & (lo_y <= y0 + 31) & (hi_y >= y0)).sum(axis=1))
    counts = np.asarray(counts)
    res["survivors_per_tile"] = {"mean": round(float(counts.mean()), 2), "max": int(counts.max()), "tiles_without_any": round(float((counts == 0).mean()), 3)}
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


def summary(trace_dir, host_json, parts_json, path):
    rows = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Name", "")
            for key in ("render_raster_kernel", "render_prims_kernel", "fill_kernel"):
                if key in name:
                    rows[key] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                                 "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    res = {"kernels": {"shape": "256 frames, N = 128 (262 primitives per frame), one 256 x 256 view: 50 331 648 output bytes; fill over the same bytes",
                       "source": "rocprofv3 --kernel-trace --stats, a run of its own (scripts/bench_render.py trace), 23 calls each", **rows},
           "raster_parts": json.load(open(parts_json)), "host": json.load(open(host_json))}
    if "render_raster_kernel" in rows and "fill_kernel" in rows:
        res["kernels"]["raster / fill"] = round(rows["render_raster_kernel"]["average_us"] / rows["fill_kernel"]["average_us"], 2)
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res["kernels"]))


if __name__ == "__main__":
    {"trace": trace, "host": host, "parts": parts, "summary": summary}[sys.argv[1]](*sys.argv[2:])
