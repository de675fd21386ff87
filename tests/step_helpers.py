"""What the tests of the step engines (mmego_amd/train_step.py) share: the recorded launches of a body, the launch STRUCTURE of a step
(tests/golden/step_structure.json, written by tests/golden/make_step_structure.py), the configurations that file covers, and every
tensor a step leaves behind (scripts/step_fingerprint.py hashes them, tests/test_step_engines_gpu.py compares graph and eager runs).

All configurations: B=4, T=8, N=128, 20 IMU samples of 15 channels, fixed seeds, LSTM dropout as the nets are constructed.  Hidden size 64
for the IMU_Nets, 256 where they run in "split3" precision (the smallest size that mode accepts)."""
import hashlib

import torch

B, T, N = 4, 8, 128
TRAINED = (("opt", "net"), ("imu_opt", "imu"), ("upper_opt", "upper_frozen"))     # (optimiser attribute, net attribute) of a step


def entry_points(body):
    """The entry-point names ``body`` launches, in order (plan.StepPlan.record: nothing is launched)."""
    from mmego_amd.plan import StepPlan
    return [n for sg in StepPlan().record(body).segments for n, _ in sg.calls]


def structure(plan):
    """A recorded plan as plain data: per segment its stream's ordinal in order of first appearance, the indices of the segments it waits
    for (resolved through the identity of their `signal` events, as StepPlan.unordered_with does) and its entry points in order; then
    the final waits as segment indices."""
    by_signal = {id(sg.signal): i for i, sg in enumerate(plan.segments) if sg.signal is not None}
    streams, segs = {}, []
    for sg in plan.segments:
        segs.append({"stream": streams.setdefault(sg.stream, len(streams)), "waits": [by_signal.get(id(ev)) for ev in sg.deps],
                     "calls": [n for n, _ in sg.calls]})
    return {"segments": segs, "final_waits": [by_signal.get(id(ev)) for ev in plan.final_waits]}


def step_structure(engine):
    """One real step (sizes the arenas and the optimiser buffers), then the structure of a whole step(): body, all-reduce, optimisers."""
    from mmego_amd.plan import StepPlan
    engine.step()
    torch.cuda.synchronize()
    return structure(StepPlan().record(engine.step))


def first_difference(name, got, want):
    """None when equal, else where the two structures of configuration ``name`` part ways first."""
    if got == want:
        return None
    for i, (a, b) in enumerate(zip(got["segments"], want["segments"])):
        for key in ("stream", "waits"):
            if a[key] != b[key]:
                return "%s: segment %d: %s %r, recorded %r" % (name, i, key, a[key], b[key])
        for j, (x, y) in enumerate(zip(a["calls"], b["calls"])):
            if x != y:
                return "%s: segment %d, launch %d: %s, recorded %s" % (name, i, j, x, y)
        if len(a["calls"]) != len(b["calls"]):
            return "%s: segment %d: %d launches, recorded %d" % (name, i, len(a["calls"]), len(b["calls"]))
    if len(got["segments"]) != len(want["segments"]):
        return "%s: %d segments, recorded %d" % (name, len(got["segments"]), len(want["segments"]))
    return "%s: final waits %r, recorded %r" % (name, got["final_waits"], want["final_waits"])


# ---- the configurations -------------------------------------------------------------------------------------------------------------------
def batch(dev, seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, N, 6, generator=g)
    x[:, ::2, 100:] = 0.0                                                        # (the loader's zero padding)
    imu = torch.randn(B, T, 20, 15, generator=g)
    body = torch.randn(B, 20, 3, generator=g) * 0.3
    target = torch.randn(B, T, 21, 3, generator=g)
    R = torch.linalg.qr(torch.randn(B, T, 3, 3, generator=g))[0].contiguous()
    return [v.to(dev) for v in (x, imu, body, target, R)]


def _upper(dev, use_graph, imu=None, wlocal=False, **kw):
    from mmego_amd import nets, nets_local
    from mmego_amd.train_step import StageStep
    x, imu_in, body, target, R = batch(dev)
    net = (nets_local.UpperNetwlocal() if wlocal else nets.UpperNet()).to(dev).train()
    if imu is not None:
        imu = nets.IMUNet(15, 9, 64, 2, True, 0).to(dev).train() if imu == "trained" else nets.IMUNet(15, 9, 64, 2).to(dev).eval()
    st = StageStep("upper", net, imu, lr=3e-5, use_graph=use_graph, finetune_imu=kw.pop("finetune_imu", False), imu_lr=1e-5, **kw)
    st.bind(x, imu_in, body, target, R_gt=None if imu is not None else R)
    return st, [net, imu]


def _lower(dev, use_graph, finetune_upper=False, wlocal=False, finetune_imu=False):
    from mmego_amd import nets, nets_local
    from mmego_amd.train_step import StageStep
    x, imu_in, body, target, R = batch(dev)
    upper = (nets_local.UpperNetwlocal() if wlocal else nets.UpperNet()).to(dev).train(finetune_upper)
    net = nets.LowerNet(64).to(dev).train()
    imu = nets.IMUNet(15, 9, 64, 2, True, 0).to(dev).train() if finetune_imu else None
    st = StageStep("lower", net, imu, upper_frozen=upper, lr=3e-5, use_graph=use_graph, finetune_upper=finetune_upper, upper_lr=1e-5,
                   finetune_imu=finetune_imu, imu_lr=1e-5)
    st.bind(x, imu_in, body, target, R_gt=None if imu is not None else R)
    return st, [net, upper, imu]


def _imu(dev, use_graph, drop):
    from mmego_amd import nets
    from mmego_amd.train_step import ImuStep
    x, imu_in, body, target, R = batch(dev)
    net = nets.IMUNet(15, 9, 64, 2, True, drop).to(dev).train()
    st = ImuStep(net, lr=1e-4, use_graph=use_graph)
    st.bind(imu_in, R, target)
    return st, [net]


def _two_stage(dev, use_graph, kind, precision="fp32"):
    from mmego_amd import nets
    from mmego_amd.train_step import ConcurrentStages, PipelinedStages, SharedImuStages, StageStep
    x, imu_in, body, target, R = batch(dev)
    H = 64 if precision == "fp32" else 256
    imu_u, imu_l = nets.IMUNet(15, 9, H, 2).to(dev).eval(), nets.IMUNet(15, 9, H, 2).to(dev).eval()
    imu_u.precision = imu_l.precision = precision
    up, lo, fr = nets.UpperNet().to(dev).train(), nets.LowerNet(64).to(dev).train(), nets.UpperNet().to(dev).eval()
    own = kind == "concurrent"
    su = StageStep("upper", up, imu_u if own else None, lr=3e-5, use_graph=False)
    sl = StageStep("lower", lo, imu_l if own else None, upper_frozen=fr, lr=3e-5, use_graph=False)
    if kind == "concurrent":
        eng = ConcurrentStages([su, sl], use_graph=use_graph)
    elif kind == "shared":
        eng = SharedImuStages(imu_u, [su, sl], imu_in, use_graph=use_graph)
    else:
        eng = PipelinedStages([su, sl], [imu_u, imu_l], imu_in, use_graph=use_graph)
    for st in (su, sl):
        st.bind(x, imu_in, body, target)
    if kind == "pipelined":
        eng.prime()
    return eng, [up, lo, fr, imu_u] + ([] if kind == "shared" else [imu_l])


CONFIGS = {
    "upper_recorded_pose": lambda dev, g: _upper(dev, g),
    "upper_frozen_imu": lambda dev, g: _upper(dev, g, imu="frozen"),
    "upper_wlocal": lambda dev, g: _upper(dev, g, wlocal=True),
    "upper_finetune_imu": lambda dev, g: _upper(dev, g, imu="trained", finetune_imu=True),
    "upper_wlocal_finetune_imu": lambda dev, g: _upper(dev, g, wlocal=True, imu="trained", finetune_imu=True),
    "upper_recorded_pose_clip": lambda dev, g: _upper(dev, g, clip_grad_norm=1.0),
    "lower_frozen_upper": lambda dev, g: _lower(dev, g),
    "lower_frozen_wlocal": lambda dev, g: _lower(dev, g, wlocal=True),
    "lower_finetune_upper": lambda dev, g: _lower(dev, g, finetune_upper=True),
    "lower_finetune_all": lambda dev, g: _lower(dev, g, finetune_upper=True, finetune_imu=True),
    "imu_step": lambda dev, g: _imu(dev, g, 0),
    "imu_step_dropout": lambda dev, g: _imu(dev, g, 0.1),
    "concurrent_fp32": lambda dev, g: _two_stage(dev, g, "concurrent"),
    "concurrent_split3": lambda dev, g: _two_stage(dev, g, "concurrent", "split3"),
    "shared_fp32": lambda dev, g: _two_stage(dev, g, "shared"),
    "pipelined_fp32": lambda dev, g: _two_stage(dev, g, "pipelined"),
    "pipelined_split3": lambda dev, g: _two_stage(dev, g, "pipelined", "split3"),
}


def build(name, dev, use_graph, seed=1000):
    """-> (engine, bound and primed; every net it runs, trained or frozen)."""
    torch.manual_seed(seed)
    eng, nets_ = CONFIGS[name](dev, use_graph)
    return eng, [m for m in nets_ if m is not None]


# ---- what a step leaves behind ------------------------------------------------------------------------------------------------------------
def trained(engine):
    """[(label, net, optimiser)] of everything the engine trains."""
    out = []
    for i, st in enumerate(getattr(engine, "stages", [engine])):
        for o, n in TRAINED:
            if getattr(st, o, None) is not None:
                out.append(("stage%d.%s" % (i, n), getattr(st, n), getattr(st, o)))
    return out


def losses(engine):
    out = []
    for st in getattr(engine, "stages", [engine]):
        out += [getattr(st, "loss2", st.loss)] + ([st.upper_loss2] if getattr(st, "upper_loss2", None) is not None else [])
    return out


def state(engine, nets_):
    """[(label, tensor)]: flat parameters and gradients and the Adam m, v, state of every trained net; every buffer (BatchNorm running
    statistics and step counters) and the seed counter of every net; the loss buffers."""
    out = []
    for tag, net, opt in trained(engine):
        out += [(tag + ".flat_p", net.flat().flat_p), (tag + ".flat_g", net.flat().flat_g)]
        out += [(tag + ".adam." + k, getattr(opt, k)) for k in ("m", "v", "state")]
    for i, net in enumerate(nets_):
        tag = "net%d.%s" % (i, type(net).__name__)
        out += [("%s.buffer.%s" % (tag, k), b) for k, b in net.named_buffers()] + [(tag + ".seed_counter", net.seed_counter())]
    return out + [("loss%d" % i, l) for i, l in enumerate(losses(engine))]


def raw(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def sha256(t):
    return hashlib.sha256(raw(t).numpy().tobytes()).hexdigest()
