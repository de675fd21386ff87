"""Fused train_once bodies of stage 2 (Upper_Net) and stage 3 (Lower_Net) on the HIP path.

Mirrors reference Processor/Train/Train_Upper.py:134-187 and Train_Lower.py:155-230 per minibatch:
frozen IMU_Net forward (eval) -> [frozen Upper_Net forward (eval)] -> trained net forward -> L1(sum) loss
-> backward -> Adam.  Differences, all host-side: no DataLoader/numpy round trip, the loss stays on the
device (no .item() sync per step), gradients live in one flat buffer (one all-reduce for data parallel,
one fused Adam launch).  Each body is capturable into a HIP graph.
"""
import contextlib
import os

import torch

from . import hip, ops
from .nets import LowerNet, UpperNet, _UpperBase
from .params import FusedAdam
from .plan import StepPlan

# A step's HIP graphs: False (the product) = the whole body as ONE graph whose parallel branches are the body's side streams; True (tests flip it) = one
# linear-chain graph per stream segment, replayed on the body's own streams with event waits in between (plan.StepPlan).  Measured
# in r03: a graph with parallel branches dispatches TINY nodes in 5-6 us against 1.5-1.8 us for linear chains in separate graphs
# (scripts/bench_launch_gap.py), but with the step's real kernels the ~15 graph boundaries cost more than that saves: 5.35 against
# 5.25 ms per U+L step, 5.11 against 5.04 ms pipelined (bit-identical results; host enqueue time 0.6 against 2.1 ms per step).
_MULTI_GRAPH = False


def _capture_body(body, stream=None):
    """-> an object with .replay(): the body as HIP graphs (no state is changed: recording / capturing executes nothing).
    ``stream``: capture under this stream (per-stream resources -- ops.scratch -- are keyed by the stream a launch was captured
    on: a graph that will run BESIDE another one needs a capture stream of its own)."""
    if _MULTI_GRAPH:
        if stream is None:
            return StepPlan().record(body).build()
        with torch.cuda.stream(stream):
            return StepPlan().record(body).build()
    g = torch.cuda.CUDAGraph()
    if stream is None:
        with ops.capture(g):
            body()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            with ops.capture(g, stream=stream):
                body()
    return g

from .skeleton import LOWER_MAP, UPPER_MAP


def allreduce_grads(flat, process_group):
    """SUM the flat gradient buffer over the ranks with ONE collective (RCCL over xGMI on the GPUs, gloo in the
    CPU tests).  The loss is a SUM over the batch, so the global-batch gradient is the SUM of the shard
    gradients -- not the mean."""
    if process_group is not None and torch.distributed.get_world_size(process_group) > 1:
        torch.distributed.all_reduce(flat.flat_g, op=torch.distributed.ReduceOp.SUM, group=process_group)


class GradBucket:
    """The flat gradient buffers of several nets back to back in ONE buffer: one all-reduce per step for all of them (the
    Upper and Lower stage of a U+L step: 1.2 + 2.5 MB -- latency-bound messages, so one collective instead of two is one
    launch + one ring latency saved per step)."""

    def __init__(self, nets):
        flats = [n.flat() for n in nets]
        sizes = [f.flat_g.numel() for f in flats]
        self.members = [id(f) for f in flats]
        self.buf = torch.zeros(sum(sizes), dtype=torch.float32, device=flats[0].flat_g.device)
        off = 0
        for f, n in zip(flats, sizes):
            f.rebind_grad(self.buf[off:off + n])
            f._bucket = self
            off += n

    @staticmethod
    def of(nets):
        """The bucket these nets already share (same nets, same order), else a new one.  Re-bucketing moves the gradient
        buffers, which would strand HIP graphs captured on the old addresses, so an existing bucket is always reused."""
        flats = [n.flat() for n in nets]
        b = getattr(flats[0], "_bucket", None)
        if b is not None and b.members == [id(f) for f in flats] and all(getattr(f, "_bucket", None) is b for f in flats):
            return b
        return GradBucket(nets)

    def allreduce(self, process_group):
        if process_group is not None and torch.distributed.get_world_size(process_group) > 1:
            torch.distributed.all_reduce(self.buf, op=torch.distributed.ReduceOp.SUM, group=process_group)


def shard_of(rank, world):
    """Slice of a global minibatch owned by ``rank`` (interleaved: balances a short last batch)."""
    return slice(rank, None, world)


def sync_replicas(net, process_group, src=0, params=True):
    """Make every rank's replica of ``net`` identical to rank ``src``'s: ONE broadcast of the flat parameter buffer (when
    ``params``) and one per registered buffer (BatchNorm running statistics, step counters, graph adjacency).  Called once when a
    data-parallel trainer starts (the nets are initialised from each rank's own RNG unless --seed is given) and once per epoch
    for the buffers alone (BatchNorm statistics are per shard, so the running averages drift apart; rank 0's are the ones
    that get saved and evaluated)."""
    if process_group is None or torch.distributed.get_world_size(process_group) < 2:
        return
    flat = net.flat()
    if params:
        torch.distributed.broadcast(flat.flat_p, src=src, group=process_group)
    seen = set()
    for b in net.buffers():
        if b.data_ptr() in seen:
            continue
        seen.add(b.data_ptr())
        torch.distributed.broadcast(b if b.dim() else b.view(1), src=src, group=process_group)


def empty_step(net, opt, process_group):
    """A rank whose shard of a short last global minibatch is empty still takes part in the step: it contributes a zero
    gradient to the all-reduce and applies the same Adam update as everybody else (otherwise the other ranks would wait
    for it forever and the replicas would part ways)."""
    flat = net.flat()
    ops.fill(flat.flat_g, 0.0)
    allreduce_grads(flat, process_group)
    opt.step()


def broadcast_flag(value, device, process_group, src=0):
    """Rank ``src``'s boolean decision (early stopping), agreed on by every rank."""
    if process_group is None or torch.distributed.get_world_size(process_group) < 2:
        return bool(value)
    t = torch.tensor([1.0 if value else 0.0], device=device)
    torch.distributed.broadcast(t, src=src, group=process_group)
    return bool(t.item() != 0.0)


def call_upper(net, x, h0, c0, body, R, t, **impl):
    """An Upper net of either kind on one zero-state pair: UpperNet takes it once, UpperNetwlocal a second time for its anchor branch
    (Net/Upper_Net.py:406-432).  Without keywords the public call ``net(...)``; with them (stash, x_src, pose_grad) ``net._forward_impl``.
    -> the net's output tuple; [0] is the 15 upper joints for both."""
    states = (h0, c0) * net.state_pairs
    if impl:
        return net._forward_impl(x, *states, body, R, t, **impl)
    return net(x, *states, body, R, t)


def needs_exclusive(nets):
    """True when one of the nets runs bf16-MFMA kernels (IMUNet.precision / train_precision, UpperNet / LowerNet.precision other than
    "fp32").  r06: a kernel that shares a CU with a bf16-MFMA workgroup of another kernel can compute wrong
    results; the cause found there (packed-fp32 instructions with op_sel) is compiled out of the library, and INDEPENDENTLY of that the
    engines keep every launch of such a step ordered against its bf16-MFMA kernels (those on one chain; only all-fp32 bodies fork, behind
    it): nothing is resident beside a bf16-MFMA workgroup but its own kernel."""
    return any(getattr(m, a, "fp32") != "fp32" for m in nets if m is not None for a in ("precision", "train_precision"))


# Everything a StageStep may train, as (optimiser attribute, net attribute), in update order.  Read LIVE wherever it is used: callers
# replace st.opt / st.imu_opt by wrappers (tests/test_clip_grad_norm_gpu.py) and step() has to call the wrapper.
TRAINED = (("opt", "net"), ("imu_opt", "imu"), ("upper_opt", "upper_frozen"))
_REFUSED = {"imu_opt": "%s: a stage with finetune_imu=True trains its IMU_Net, which is then no frozen, shareable forward; run it as a "
                       "plain StageStep",
            "upper_opt": "%s: a stage with finetune_upper=True trains its Upper_Net inside its own body (two nets, two optimisers); run it "
                         "as a plain StageStep"}


def _refuse_finetune(who, stages):
    """The multi-stage engines run FROZEN IMU_Nets (shared, prefetched or beside another stage) and one optimiser per stage: a stage that
    trains more than its own net does not fit."""
    for o, _ in TRAINED[1:]:
        if any(getattr(st, o, None) is not None for st in stages):
            raise ValueError(_REFUSED[o] % who)


class _Engine:
    """What every step engine is: the capture protocol and step().  An engine supplies its ``_body``, the tensors the body changes besides
    gradients and activations (``_mutable_state``), the number of warm-up runs ahead of a capture (``warm_ups``) and its ``_update``."""
    warm_ups = 1
    graph = None

    def warm_up(self):
        """Run the body WITHOUT side effects (sizes the arenas, sets kernel attributes before graph capture): the mutable state is put
        back afterwards, so graph and eager runs -- and a resumed run -- see identical states."""
        keep = [t.clone() for t in self._mutable_state()]
        for _ in range(self.warm_ups):
            self._body()
            torch.cuda.synchronize()
        for t, k in zip(self._mutable_state(), keep):
            t.copy_(k)
        torch.cuda.synchronize()

    def prepare(self):
        """Size the arenas and capture the HIP graph without changing any state (so that the first step() costs what every step costs)."""
        if self.use_graph and self.graph is None:
            self.warm_up()
            self.graph = _capture_body(self._body)

    def step(self):
        if self.use_graph:
            self.prepare()
            self.graph.replay()
        else:
            self._body()
        self._update()
        return self._losses()

    # -- an engine around ONE trained net and its flat gradient buffer (StageStep, ImuStep) ---------------------------------------
    def optimisers(self):
        return [opt for opt in (getattr(self, o, None) for o, _ in TRAINED) if opt is not None]

    def _update(self):
        allreduce_grads(self.net._flat, self.pg)
        for opt in self.optimisers():
            opt.step()

    def _losses(self):
        return self.loss

    # -- imu_noise: the IMU samples perturbed on their way into the engine's IMU_Net (StageStep, ImuStep) ------------------------------
    imu_noise = None

    def _init_imu_noise(self, imu_noise, dev):
        """``imu_noise`` checked and kept as six floats, with the device word of the draws and the output buffers per bound shape."""
        if imu_noise is None:
            return
        try:
            sig = tuple(float(v) for v in imu_noise)
        except (TypeError, ValueError):
            sig = ()
        if len(sig) != 6 or not all(0.0 <= v < float("inf") for v in sig) or not any(sig):
            raise ValueError("%s: imu_noise is (noise_rot_deg, noise_acc, noise_gyro, bias_rot_deg, bias_acc, bias_gyro), finite and >= 0, "
                             "one of them > 0, got %r" % (type(self).__name__, imu_noise))
        self.imu_noise = sig
        self.imu_word = torch.zeros(1, dtype=torch.int64, device=dev)       # the draws' key: set_imu_key
        self._imu_out = {}                                                  # the bound samples' shape -> their perturbed copy

    def set_imu_key(self, k):
        """The key of the next step's IMU noise and bias draws (its low 63 bits): written between steps, outside the graph."""
        self.imu_word.fill_(int(k) & 0x7FFFFFFFFFFFFFFF)

    def _bind_imu_out(self, imu):
        if self.imu_noise is not None and tuple(imu.shape) not in self._imu_out:
            self._imu_out[tuple(imu.shape)] = torch.empty_like(imu)

    def _imu_samples(self, s):
        """The minibatch's IMU samples as the IMU_Net gets them: the bound buffer, or under imu_noise its perturbed copy in the engine's
        own buffer (one mmego_imu_jitter launch, part of the body; the bound buffer is never written)."""
        if self.imu_noise is None:
            return s["imu"]
        return ops.imu_jitter(s["imu"], self.imu_noise, self.imu_word, self._imu_out[tuple(s["imu"].shape)])


class _StagesEngine(_Engine):
    """An engine around several StageSteps (``stages``) whose gradients ``pair`` all-reduces: each stage trains its one net."""

    def _mutable_state(self):
        return [t for st in self.stages for t in st._mutable_state()]

    def _update(self):
        self.pair.allreduce()
        for st in self.stages:
            for opt in st.optimisers():
                opt.step()

    def _losses(self):
        return [st.loss for st in self.stages]


class StageStep(_Engine):
    """One training stage's per-minibatch body with static buffers (graph friendly).

    ``imu_net=None`` takes the head pose from the recording (R_gt, ground-truth head joint) instead of the
    frozen IMU_Net -- the shipped reference snapshot has no IMU_Net checkpoint.

    ``finetune_imu`` (Upper stage): the IMU_Net is trained too, through the pose loss -- Train_Upper.py:162 without its .detach().
    Per minibatch: IMU_Net training forward -> R, t -> Upper_Net forward + loss + backward, which now leaves d loss / d R and
    d loss / d t (UpperNet.pose_grads) -> IMU_Net backward -> two Adam steps (Upper_Net at ``lr``, IMU_Net at ``imu_lr`` with stage
    1's weight decay).  The body is still one HIP graph.  The trained net is an UpperNet or an UpperNetwlocal.

    ``upper_frozen`` (Lower stage): a frozen UpperNet or UpperNetwlocal (``call_upper``); the options that TRAIN it take an UpperNet only.

    ``finetune_upper`` (Lower stage): joint stage-3 training -- Train_Lower.py:195-196 without its .detach().  ``upper_frozen`` is then
    NOT frozen: per minibatch it runs a TRAIN-mode forward that keeps its activations, with its own L1(sum) loss on the 15 upper joints
    (``upper_loss2``); Lower_Net's forward takes that prediction undetached, its backward leaves d loss_lower / d upper_l
    (LowerNet.input_grads), and Upper_Net's backward runs on d(loss_lower + loss_upper); two Adam steps (Lower_Net at ``lr``, Upper_Net at
    ``upper_lr``, default ``lr``).  The head pose is not trained (frozen IMU_Net, shared pose or the recording, as without the option).
    The sum of the two stages' own losses, because the final skeleton takes 13 of its 21 joints from Upper_Net: the lower loss alone must
    not be the only thing steering it.  One HIP graph.

    ``finetune_upper`` AND ``finetune_imu`` (Lower stage): the three-net step.  IMU_Net training forward -> R, t -> Upper_Net train-mode
    forward (own loss, pose_grad) -> Lower_Net train-mode forward on that prediction and the same R, t (input_grad upper_l + pose) ->
    loss_lower + loss_upper; backward: Lower_Net leaves d upper_l, dR_L, dt_L; Upper_Net runs on its own loss gradient plus d upper_l and
    leaves dR, dt = world transform of its own loss + world transform of d upper_l + Lower_Net's dR_L, dt_L (those three from ONE launch,
    mmego_head_fk_backward_extra) + its head-frame transform; IMU_Net backward on that sum; three Adam steps (Lower_Net at ``lr``,
    Upper_Net at ``upper_lr``, IMU_Net at ``imu_lr`` with stage 1's weight decay).  IMU_Net has no loss term of its own.  Lower_Net's
    POINT input stays data: the points it gets were transformed once by Upper_Net in place (Q1), and that transform's dependence on R, t
    is not differentiated (LowerNet.differentiable_inputs: "x gets none").  One HIP graph; not data parallel.

    ``clip_grad_norm`` (None: off): every optimiser this step builds -- ``opt``, ``imu_opt``, ``upper_opt`` -- clips ITS net's gradient
    to that global norm ahead of its update (FusedAdam(max_grad_norm=...)): one clip_grad_norm_ per optimiser, as the nets have separate
    optimisers and learning rates.  Data parallel, the all-reduce precedes ``opt.step()``: every rank clips the summed gradient by the
    same norm.

    ``ema_decay`` (None: off): every optimiser this step builds keeps an exponential moving average of ITS net's weights at that decay
    (FusedAdam(ema_decay=...)), updated inside its own Adam launch -- which runs outside the captured body, so the graph is the one
    without the option.  Data parallel, no collective: replicas with bit-equal parameters compute bit-equal averages.

    ``lr_schedule`` (None: a constant rate; else a params.LrSchedule): every optimiser this step builds gets the SAME schedule over its
    own base rate (``lr``, ``imu_lr``, ``upper_lr``) and computes its rate inside its own Adam launch from its own step count
    (FusedAdam(lr_schedule=...)): the nets of a fine-tuning step warm up and decay together.  Data parallel, no collective: the step
    counts of the ranks agree -- the clipped form decides to skip on the all-reduced gradient, which precedes ``opt.step()``.

    ``optimisers`` (a dict keyed "opt" / "imu_opt" / "upper_opt"): the ones in it are used as they are, the missing ones are built and
    put into it -- a trainer hands ONE dict to the steps of all its minibatch sizes, so every optimiser is built once.

    ``pose_noise_deg`` / ``pose_noise_t`` (None: off; either alone is fine): the head pose the stage's nets get -- the recording's, the
    frozen IMU_Net's, or the shared / prefetched ``pose`` buffers -- is perturbed per frame inside the body by one mmego_pose_jitter
    launch (ops.pose_jitter: a rotation vector of standard deviation pose_noise_deg degrees per axis, a shift of pose_noise_t per
    component), OUT of place into a pair of buffers the step owns per bound minibatch size: warm_up runs the body more than once on
    the same inputs, and noise applied in place would compound.  The draw is a function of ``pose_word``, an int64 device word the
    kernel reads: callers write it between steps with ``set_pose_key(k)``, outside the graph, so every replay draws afresh and a
    resumed run continues the sequence.  The engines around a stage run it unchanged: the launch is part of the stage's body, and
    each stage has its own word.  There is no backward through the perturbation: a stage that TRAINS the pose (finetune_imu, with or
    without finetune_upper) refuses the options; finetune_upper alone is fine, its pose is data.  With both None the step launches
    what it launched before and owns no extra buffer.

    ``imu_noise`` (None: off; else (noise_rot_deg, noise_acc, noise_gyro, bias_rot_deg, bias_acc, bias_gyro), finite and >= 0, one of them
    > 0): the IMU samples the stage's OWN IMU_Net reads -- trained (finetune_imu: imu_train.forward_train) or frozen -- are perturbed
    inside the body by one mmego_imu_jitter launch (ops.imu_jitter: white noise per sample, a bias constant over each window), OUT of
    place into a buffer the step owns per bound minibatch shape; the bound buffer is never written.  The draws are a function of
    ``imu_word``, an int64 device word the kernel reads: callers write it between steps with ``set_imu_key(k)``, outside the graph.  The
    gradient flows as it did: the perturbation sits in front of the net's input, which is data.  A stage with no IMU_Net of its own --
    the recorded pose, or a ``pose`` shared or prefetched by somebody else (SharedImuStages, PipelinedStages) -- has nothing to perturb
    and refuses the option, at construction or when such a ``pose`` is assigned.  With None the step launches what it launched before
    and owns no extra buffer.

    ``decoupled`` / ``no_decay`` (False / None: the coupled decay over every tensor): FusedAdam's options of those names, handed to every
    optimiser this step builds -- ``no_decay`` is "1d" or names; a list of names has to fit every trained net, so several nets take "1d".
    The decay of each net stays ``weight_decay`` / ``imu_weight_decay``.  With the defaults every optimiser makes the calls it made."""

    def __init__(self, stage, net, imu_net, upper_frozen=None, lr=3e-5, weight_decay=0.0, process_group=None,
                 use_graph=True, pose=None, finetune_imu=False, imu_lr=None, imu_weight_decay=0.001, finetune_upper=False, upper_lr=None,
                 clip_grad_norm=None, optimisers=None, ema_decay=None, pose_noise_deg=None, pose_noise_t=None,
                 lr_schedule=None, imu_noise=None, decoupled=False, no_decay=None):
        assert stage in ("upper", "lower")
        if imu_noise is not None and (imu_net is None or pose is not None):
            raise ValueError("StageStep: imu_noise perturbs what the stage's own IMU_Net reads; this stage has none (the recorded or a "
                             "shared head pose)")
        self.pose_noise = None
        if pose_noise_deg is not None or pose_noise_t is not None:
            if finetune_imu:
                raise ValueError("StageStep: pose_noise_deg / pose_noise_t perturb a head pose that is DATA; finetune_imu trains it, and "
                                 "there is no backward through the perturbation")
            sig = tuple(0.0 if v is None else float(v) for v in (pose_noise_deg, pose_noise_t))
            if not all(0.0 <= v < float("inf") for v in sig) or sig == (0.0, 0.0):
                raise ValueError("StageStep: pose_noise_deg / pose_noise_t are finite and >= 0, one of them > 0, got %r, %r"
                                 % (pose_noise_deg, pose_noise_t))
            self.pose_noise = sig
        self.stage, self.net, self.imu, self.upper_frozen = stage, net, imu_net, upper_frozen
        self._pose = pose             # (R, t) device buffers filled by somebody else (the "IMU-shared" arrangement): the ``pose`` property
        self.finetune_imu = bool(finetune_imu)
        self.finetune_upper = bool(finetune_upper)
        opts = {} if optimisers is None else optimisers

        def opt_for(key, trained, lr, weight_decay):
            if opts.get(key) is None:
                opts[key] = FusedAdam(trained.flat(), lr=lr, weight_decay=weight_decay, max_grad_norm=clip_grad_norm, ema_decay=ema_decay,
                                      lr_schedule=lr_schedule, decoupled=decoupled, no_decay=no_decay)
            return opts[key]
        self.imu_opt = self.upper_opt = None
        if self.finetune_upper:
            if stage != "lower" or type(net) is not LowerNet:
                raise ValueError("StageStep: finetune_upper trains Upper_Net through Lower_Net's input gradients: the Lower stage only")
            if type(upper_frozen) is not UpperNet:
                raise ValueError("StageStep: finetune_upper needs the Upper_Net to train as upper_frozen (a plain UpperNet; UpperNetwlocal "
                                 "is not supported)")
            if self.finetune_imu and (imu_net is None or pose is not None):
                raise ValueError("StageStep: finetune_upper with finetune_imu (the three-net step) needs an IMU_Net of its own to train "
                                 "(no recorded or shared head pose)")
            if process_group is not None and torch.distributed.get_world_size(process_group) > 1:
                raise ValueError("StageStep: finetune_upper is not data parallel yet (no all-reduce of the Upper_Net gradients)")
            self.upper_opt = opt_for("upper_opt", upper_frozen, lr if upper_lr is None else upper_lr, weight_decay)
        if self.finetune_imu:
            if not self.finetune_upper and (stage != "upper" or not isinstance(net, _UpperBase)):
                raise ValueError("StageStep: finetune_imu trains IMU_Net through the head-pose gradients of the Upper stage's net (UpperNet "
                                 "or UpperNetwlocal); Lower_Net's (LowerNet.input_grads) reach it through a trained Upper_Net only "
                                 "(finetune_upper as well: the three-net step)")
            if imu_net is None or pose is not None:
                raise ValueError("StageStep: finetune_imu needs an IMU_Net of its own (no recorded or shared head pose)")
            if process_group is not None and torch.distributed.get_world_size(process_group) > 1:
                raise ValueError("StageStep: finetune_imu is not data parallel yet (no all-reduce of the IMU_Net gradients)")
            self.imu_opt = opt_for("imu_opt", imu_net, lr if imu_lr is None else imu_lr, imu_weight_decay)
        self.opt = opt_for("opt", net, lr, weight_decay)
        self.pg = process_group
        self.use_graph = use_graph
        self.graph = None
        self.static = None
        dev = next(net.parameters()).device
        self.jmap = torch.tensor(UPPER_MAP if stage == "upper" else LOWER_MAP, dtype=torch.int32, device=dev)
        self.loss2 = torch.zeros(2, dtype=torch.float32, device=dev)   # [L1 sum, sum of per-joint Euclidean distances]
        self.loss = self.loss2[:1]
        self.last_pred = None
        if self.pose_noise is not None:
            self.pose_word = torch.zeros(1, dtype=torch.int64, device=dev)      # the draw's key: set_pose_key
            self._pose_out = {}                                        # (B, T) -> (R_n, t_n)
        self._init_imu_noise(imu_noise, dev)
        if self.finetune_upper:                                        # (loss2 stays the Lower stage's pair: the trainers log it)
            self.upper_jmap = torch.tensor(UPPER_MAP, dtype=torch.int32, device=dev)
            self.upper_loss2 = torch.zeros(2, dtype=torch.float32, device=dev)

    @property
    def pose(self):
        return self._pose

    @pose.setter
    def pose(self, pose):
        """The engines that fill the pose for a stage assign it here: under imu_noise that would drop the noise without a word."""
        if pose is not None and self.imu_noise is not None:
            raise ValueError("StageStep: imu_noise perturbs what the stage's own IMU_Net reads; a shared or prefetched head pose bypasses it")
        self._pose = pose

    def _body(self):
        self._body_forward()
        self._body_backward()

    def _body_forward(self):
        """Fresh batch, head pose, forward of the trained net (and of the frozen Upper_Net in the Lower stage), loss."""
        s = self.static
        B, T = s["x"].shape[0], s["x"].shape[1]
        first_net = self.net if self.stage == "upper" else self.upper_frozen
        # fresh batch (x is transformed in place): an Upper net's transform launch reads it from x_src; other nets get a copy first
        via_transform = isinstance(first_net, _UpperBase) and s["x"].shape[-1] <= 8
        # the trained net's kinematics launch takes the loss, its gradient and the first backward step along (nets._head_fk)
        self.net.loss_hook = (s["target"], self.jmap, self.loss2, 1.0)
        if self.finetune_upper:
            self.upper_frozen.loss_hook = (s["target"], self.upper_jmap, self.upper_loss2, 1.0)
        try:
            with torch.no_grad():
                self._body_forward_inner(s, B, T, via_transform)
        finally:
            self.net.loss_hook = None
            if self.finetune_upper:
                self.upper_frozen.loss_hook = None

    def set_pose_key(self, k):
        """The key of the next step's head-pose draw (its low 63 bits): written between steps, outside the graph."""
        self.pose_word.fill_(int(k) & 0x7FFFFFFFFFFFFFFF)

    def _head_pose(self, s, B, T):
        """(R, t) of the minibatch: the trained IMU_Net's, the shared pose, the frozen IMU_Net's, or the recording's -- under pose_noise_deg /
        pose_noise_t the perturbed copy of it in the step's own buffers."""
        R, t = self._clean_head_pose(s, B, T)
        if self.pose_noise is None:
            return R, t
        R_n, t_n = self._pose_out[(B, T)]
        return ops.pose_jitter(R.contiguous().view(B, T, 3, 3), t.contiguous().view(B, T, 3), self.pose_noise[0], self.pose_noise[1],
                               self.pose_word, R_n, t_n)

    def _clean_head_pose(self, s, B, T):
        """The pose as its source gives it."""
        if self.finetune_imu:
            from . import imu_train
            return imu_train.forward_train(self.imu, self._imu_samples(s))
        if self.pose is not None:
            return self.pose
        if self.imu is not None:
            return self.imu(self._imu_samples(s))
        ops.copy2d(s["target"].view(B * T, 63)[:, 60:63], s["t_gt"].view(B * T, 3))
        return s["R_gt"], s["t_gt"]

    def _l1_fallback(self, net, pred, jmap, nsel, loss2, dl):
        """The loss as a launch of its own, where ``net``'s kinematics launch did not take it along (nets._head_fk: no fused form)."""
        if not getattr(net, "_dy_ready", False):
            s = self.static
            hip.call("l1_loss", pred, s["target"], jmap, nsel, 21, s["x"].shape[0] * s["x"].shape[1], 1.0, loss2, dl)

    def _body_forward_inner(self, s, B, T, via_transform):
        if not via_transform:
            ops.copy2d(s["x_src"].view(B * T, -1), s["x"].view(B * T, -1))
        x_src = s["x_src"] if via_transform else None       # (without x_src the net keeps its own copy of the untransformed points)
        R, t = self._head_pose(s, B, T)
        if self.stage == "upper":
            pose_grad = {"pose_grad": True} if self.finetune_imu else {}      # (only a trained IMU_Net consumes d loss / d R, d loss / d t)
            l = call_upper(self.net, s["x"], s["h0"], s["c0"], s["body"], R, t, stash=True, x_src=x_src, **pose_grad)[0]
            nsel = 15
        else:
            upper = self.upper_frozen
            if self.finetune_upper and not upper.training:
                raise ValueError("StageStep: finetune_upper needs its Upper_Net in train mode (call .train() on it)")
            if self.finetune_upper or (via_transform and not upper.training):
                # (trained: a train-mode forward that keeps its activations; frozen: the eval forward)
                pose_grad = {"pose_grad": True} if self.finetune_imu else {}      # (the three-net step: Upper_Net hands dR, dt to IMU_Net)
                up = call_upper(upper, s["x"], s["h0"], s["c0"], s["body"], R, t, stash=self.finetune_upper, x_src=x_src, **pose_grad)[0]
            else:
                if via_transform:
                    ops.copy2d(s["x_src"].view(B * T, -1), s["x"].view(B * T, -1))
                up = call_upper(upper, s["x"], s["h0"], s["c0"], s["body"], R, t)[0]
            if self.finetune_upper:
                self._l1_fallback(upper, up, self.upper_jmap, 15, self.upper_loss2, s["dl_up"])
                self.last_upper_pred = up
            # (the three-net step: Lower_Net's own pose gradients as well -- its two head-frame transforms and its world transform; the
            #  points it receives, transformed once by Upper_Net, stay data)
            want = (("upper_l", "pose") if self.finetune_imu else ("upper_l",)) if self.finetune_upper else ()
            l = self.net._forward_impl(up, s["x"], s["body"], R, t, stash=True, input_grad=want)[0]
            nsel = 8
        self._l1_fallback(self.net, l, self.jmap, nsel, self.loss2, s["dl"])
        self.last_pred = l

    def _body_backward(self):
        with torch.no_grad():
            self.net._backward_impl(self.static["dl"])
            if self.finetune_upper:
                # d(loss_lower + loss_upper) / d(Upper_Net's joints): its own loss's share and Lower_Net's d upper_l
                d_up, dR_l, dt_l = self.net.input_grads()
                # (the three-net step: Lower_Net's dR, dt join Upper_Net's three shares there)
                self.upper_frozen._backward_impl(self.static["dl_up"], dl_extra=d_up, pose_add=(dR_l, dt_l) if self.finetune_imu else None)
            if self.finetune_imu:
                from . import imu_train
                imu_train.backward(self.imu, *(self.upper_frozen if self.finetune_upper else self.net).pose_grads())

    def bind(self, x, imu, body, target, R_gt=None):
        """Register the (device-resident) minibatch buffers; contents may be overwritten between steps."""
        dev = x.device
        B, T = x.shape[0], x.shape[1]
        nsel = 15 if self.stage == "upper" else 8
        if self.imu is None and R_gt is None and self.pose is None:
            raise ValueError("StageStep without an IMU_Net needs the recorded head rotations (R_gt)")
        self.static = dict(x_src=x, x=torch.empty_like(x), imu=imu, body=body, target=target,
                           h0=torch.zeros(6, B, 64, device=dev), c0=torch.zeros(6, B, 64, device=dev),
                           dl=torch.empty(B, T, nsel, 3, device=dev), R_gt=R_gt,
                           t_gt=torch.empty(B, T, 3, device=dev))
        if self.finetune_upper:
            self.static["dl_up"] = torch.empty(B, T, 15, 3, device=dev)
        if self.pose_noise is not None and (B, T) not in self._pose_out:
            self._pose_out[(B, T)] = (torch.empty(B, T, 3, 3, device=dev), torch.empty(B, T, 3, device=dev))
        self._bind_imu_out(imu)
        self.graph = None

    def _mutable_state(self):
        """What a body changes besides gradients/activations: BatchNorm running statistics + step counters and the dropout
        counter of the trained net(s) (the frozen nets run in eval mode)."""
        nets = [getattr(self, n) for o, n in TRAINED if getattr(self, o) is not None]
        return [t for net in nets for t in list(net.buffers()) + [net.seed_counter()]]


class ImuStep(_Engine):
    """Stage-1 per-minibatch body (reference Processor/Train/Train_IMU.py:114-149): IMU_Net forward, geodesic + 100 x
    position loss (sum), backward through the two BiLSTM(512) stacks, Adam with coupled weight decay -- with static
    buffers, capturable into one HIP graph (the eager body is ~650 launches and CPU-launch bound).

    ``imu_noise`` (None: off): StageStep's option of that name -- the bound IMU samples are perturbed by one mmego_imu_jitter launch in
    front of the net's forward, out of place into a buffer the step owns per bound shape, under the device word ``imu_word`` that
    ``set_imu_key(k)`` writes between steps.  With None the step launches what it launched before and owns no extra buffer."""

    def __init__(self, net, lr=1e-4, weight_decay=0.001, process_group=None, use_graph=True, clip_grad_norm=None, opt=None, ema_decay=None,
                 lr_schedule=None, imu_noise=None, decoupled=False, no_decay=None):
        self.net = net
        # (clip_grad_norm, ema_decay, lr_schedule, decoupled, no_decay: of the optimiser built here -- FusedAdam(max_grad_norm=..., ema_decay=...,
        #  lr_schedule=..., decoupled=..., no_decay=...); one handed in is used as it is)
        self.opt = opt if opt is not None else FusedAdam(net.flat(), lr=lr, weight_decay=weight_decay, max_grad_norm=clip_grad_norm,
                                                         ema_decay=ema_decay, lr_schedule=lr_schedule, decoupled=decoupled, no_decay=no_decay)
        self.pg = process_group
        self.use_graph = use_graph
        self.graph = None
        self.static = None
        dev = next(net.parameters()).device
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self._init_imu_noise(imu_noise, dev)

    def bind(self, imu, R_gt, target):
        dev = imu.device
        B, T = imu.shape[0], imu.shape[1]
        self.static = dict(imu=imu, R_gt=R_gt, target=target, head=torch.empty(B, T, 3, device=dev),
                           dR=torch.empty(B, T, 3, 3, device=dev), dt=torch.empty(B, T, 3, device=dev))
        self._bind_imu_out(imu)
        self.graph = None

    def _body(self):
        from . import imu_train
        s = self.static
        B, T = s["imu"].shape[0], s["imu"].shape[1]
        with torch.no_grad():
            ops.copy2d(s["target"].view(B * T, 63)[:, 60:63], s["head"].view(B * T, 3))     # head joint = joint 20
            R, t = imu_train.forward_train(self.net, self._imu_samples(s))
            hip.call("imu_loss", R, t, s["R_gt"], s["head"], B * T, 1.0, self.loss, s["dR"], s["dt"])
            imu_train.backward(self.net, s["dR"], s["dt"])

    def _mutable_state(self):
        return [self.net.seed_counter()]                       # (IMU_Net has no BatchNorm: the dropout counter is all a body changes)


class SharedImuStages(_StagesEngine):
    """The "IMU-shared" arrangement of SURVEY 8-d: ONE frozen IMU_Net forward per minibatch feeds both stage bodies (they
    run as two concurrent branches after it).  Not what the reference does (each stage program runs its own IMU_Net
    forward); reported beside the literal U+L step."""
    warm_ups = 2          # the bodies fork: the second run sizes the side streams' scratch (ops.scratch is keyed by capture stream)

    def __init__(self, imu_net, stages, imu_in, use_graph=True):
        self.imu, self.stages, self.imu_in = imu_net, list(stages), imu_in
        _refuse_finetune("SharedImuStages", self.stages)
        B, T = imu_in.shape[0], imu_in.shape[1]
        dev = imu_in.device
        self.R, self.t = torch.empty(B, T, 3, 3, device=dev), torch.empty(B, T, 3, device=dev)
        for st in self.stages:
            st.pose = (self.R, self.t)
        self.pair = ConcurrentStages(self.stages, use_graph=False)
        self.pair.extra_nets = [self.imu]
        self.use_graph, self.graph = use_graph, None

    def _body(self):
        with torch.no_grad(), (ops.no_fork() if self.pair.exclusive() else contextlib.nullcontext()):
            R, t = self.imu(self.imu_in)
            ops.copy2d(R.view(-1, 9), self.R.view(-1, 9))
            ops.copy2d(t.view(-1, 3), self.t.view(-1, 3))
        self.pair._bodies()


class ConcurrentStages(_StagesEngine):
    """Several INDEPENDENT stage bodies per minibatch as concurrent branches of one HIP graph.

    In the reference the Upper and Lower stages are separate programs (Train_Lower.py:129-137 loads a frozen, already
    trained Upper_Net; nothing flows from one body to the other), so their per-minibatch bodies may run side by side.
    On the GPU that matters: half of a body is IMU_Net's compute-bound products, the other half is hundreds of small
    latency-bound kernels that leave most CUs idle; interleaving two bodies fills those CUs (measured: 8.2 -> 7.1 ms
    per U+L step).  Each stage must own its buffers: in particular each needs its OWN frozen IMU_Net instance (the
    nets keep their activations in per-instance arenas).  Results are bit-identical to running the stages one after
    the other (every reduction in the kernels has a fixed order)."""

    def __init__(self, stages, use_graph=True, unguarded=False):
        self.stages = list(stages)
        _refuse_finetune("ConcurrentStages", self.stages)
        # unguarded: keep the concurrent branches even when a net runs bf16-MFMA kernels (bench.py's comparison figure and the
        # reproducers of scripts/ only; see needs_exclusive)
        self.unguarded = unguarded
        nets_used = [id(m) for st in self.stages for m in (st.net, st.imu, st.upper_frozen) if m is not None]
        if len(set(nets_used)) != len(nets_used):
            raise ValueError("ConcurrentStages: stages share a network instance (each stage needs its own IMU_Net / "
                             "frozen Upper_Net copy: their activation arenas would be written concurrently)")
        self.use_graph = use_graph
        self.graph = None
        self.extra_nets = []                                  # nets that run beside the stages without being theirs (the owner's IMU_Nets)
        self.side = [torch.cuda.Stream() for _ in self.stages[1:]]
        # data parallel: the stages' gradients share one buffer, so one collective per step serves all of them
        self.bucket = None
        pgs = {id(st.pg) for st in self.stages}
        pg = self.stages[0].pg
        if len(pgs) == 1 and pg is not None and torch.distributed.get_world_size(pg) > 1 and len(self.stages) > 1:
            self.bucket = GradBucket.of([st.net for st in self.stages])

    @property
    def pair(self):
        """The engines built around a ConcurrentStages call theirs `pair`; this one is its own.  (A property, not an attribute: a
        reference to itself would leave a dropped engine -- and its HIP graph -- to the cyclic collector, which may run inside somebody
        else's capture, where destroying a graph is an error.)"""
        return self

    def allreduce(self):
        if self.bucket is not None:
            self.bucket.allreduce(self.stages[0].pg)
        else:
            for st in self.stages:
                allreduce_grads(st.net._flat, st.pg)

    def exclusive(self):
        """One chain instead of branches: a net of a stage (or one handed in by PipelinedStages / SharedImuStages) runs bf16 MFMAs."""
        return not self.unguarded and needs_exclusive([m for st in self.stages for m in (st.net, st.imu, st.upper_frozen)] + list(self.extra_nets))

    def _bodies(self):
        if not self.exclusive():
            return self._bodies_concurrent()
        # A net runs bf16 MFMAs (needs_exclusive): everything that may launch such a kernel goes onto ONE chain -- the frozen IMU_Net
        # forwards first, one after the other, every fork site inside them closed (ops.no_fork) -- and only bodies whose own nets are
        # all fp32 fork off behind it (one stage's tail beside the other's: neither holds a bf16-MFMA kernel).  Bodies with such a net
        # (a frozen Upper_Net in bf16 precision) stay on the chain as well.  The structural test reads exactly this off the recorded
        # launch graph (tests/test_split3_gpu.py::test_no_kernel_can_run_beside_a_bf16_mfma_kernel).
        main = torch.cuda.current_stream()
        stages = self.stages
        keep = [(st.imu, st.pose) for st in stages]
        try:
            with ops.no_fork(), torch.no_grad():
                for st in reversed(stages):
                    if st.imu is not None and st.pose is None:
                        st.pose = st.imu(st.static["imu"])
            hot_bodies = needs_exclusive([m for st in stages for m in (st.net, st.upper_frozen)])
            if hot_bodies or len(stages) == 1 or not ops.capture_can_fork():
                with ops.no_fork():
                    for st in reversed(stages):               # (the order of the branch form; the results do not depend on it)
                        st._body()
            else:
                for i in range(len(stages) - 1, 0, -1):
                    self.side[i - 1].wait_stream(main)
                    with torch.cuda.stream(self.side[i - 1]):
                        stages[i]._body()
                stages[0]._body()
                for side in self.side:
                    main.wait_stream(side)
        finally:
            for st, (imu, pose) in zip(stages, keep):
                st.imu, st.pose = imu, pose

    def _bodies_concurrent(self):
        """Branch order: the LAST stage (longest tail: the Lower body also runs the frozen Upper_Net) gets its IMU_Net forward
        first, alone on the GPU, with its recurrences as two single-direction chains (blocks.two_chains); each earlier stage's
        IMU_Net forward follows on the launching stream when that one has finished, with the previous stage's small-kernel tail
        beside it; each stage's remaining body forks off right after its own forward and takes the head pose from a per-stage
        buffer.  The IMU_Net forwards are compute-bound and gain nothing from running side by side, whereas the small-kernel
        tail of one stage overlaps with the IMU_Net forward of another (measured: 6.88 -> 6.54 ms per U+L step).  Other
        arrangements that were measured and dropped: NOTES.md."""
        main = torch.cuda.current_stream()
        stages, streams = self.stages, [main] + self.side
        keep = [(st.imu, st.pose) for st in stages]
        try:
            for i in range(len(stages) - 1, -1, -1):
                st = stages[i]
                if st.imu is not None and st.pose is None:
                    from . import blocks
                    # the FIRST forward (the last stage's) has the GPU to itself: its recurrences run as two chains; the
                    # later ones have another stage's tail beside them, which fills the same gaps (blocks.two_chains)
                    # r03: with the shorter tails the later forwards gain from the two-chain form as well (5.30 -> 5.24 ms per
                    # U+L step), so all of them take it
                    with torch.no_grad(), blocks.two_chains(True):
                        # (the forward's own output tensors serve as the stage's head pose: they stay referenced -- and, under
                        # capture, reserved in the graph's pool -- until every branch has been enqueued; no copies)
                        st.pose = st.imu(st.static["imu"])
                if i > 0:
                    streams[i].wait_stream(main)
                    with torch.cuda.stream(streams[i]):
                        st._body()
                else:
                    st._body()
        finally:
            for st, (imu, pose) in zip(stages, keep):
                st.imu, st.pose = imu, pose
        for side in self.side:
            main.wait_stream(side)

    def _body(self):
        self._bodies()

    def warm_up(self):
        for st in self.stages:                              # each stage alone first: sizes its arenas, sets its kernel attributes
            st.warm_up()
        super().warm_up()                                   # then all of them: the per-stream scratch buffers of the side streams


class PipelinedStages(_StagesEngine):
    """ConcurrentStages with the frozen IMU_Net forwards moved one minibatch ahead (a prefetch pipeline).

    The IMU_Net forwards of a stage body depend on nothing the step changes (frozen weights, the minibatch's IMU samples), so
    the forwards for minibatch i+1 can run while the trainable bodies work on minibatch i: the compute-bound half of a body
    overlaps the latency-bound half of the previous one.  One replay = [head poses of minibatch i move from the "next" to the
    "current" buffers] -> {Upper body(i) | Lower body(i) | IMU_Net_L(i+1) | IMU_Net_U(i+1)} as four concurrent branches: the two
    forwards run SIDE BY SIDE (each on a stream of its own, forked from the capture's origin), so that one net's recurrent step
    fills the launch gap / prologue / cell update of the other's -- 19.3 us per timestep and net instead of 23.4 (bench.py
    `recurrence_graph`), 5.18 ms per U+L step instead of 5.48 with the two forwards one after the other in ONE branch
    (side_by_side = False).  Within one minibatch the same pairing loses (both tails then start together, NOTES.md); across minibatches nothing waits for the forwards.
    Every step still runs both IMU_Net forwards in full; results are bit-identical to ConcurrentStages on the same sequence of
    minibatches (tests/test_hip_local.py).  `imu_next` is the static buffer the caller fills with minibatch i+1's IMU samples
    before step i; `prime()` runs the forwards for the first minibatch."""
    warm_ups = 2          # side streams: the second run sizes their scratch (ops.scratch is keyed by capture stream)

    def __init__(self, stages, imu_nets, imu_next, use_graph=True, unguarded=False):
        self.stages, self.imus, self.imu_next = list(stages), list(imu_nets), imu_next
        _refuse_finetune("PipelinedStages", self.stages)
        if len(self.stages) != len(self.imus) or any(st.imu is not None for st in self.stages):
            raise ValueError("PipelinedStages: one IMU_Net per stage, and the stages themselves must be built with imu_net=None")
        if len({id(m) for m in self.imus}) != len(self.imus):
            raise ValueError("PipelinedStages: every stage needs its own IMU_Net instance")
        B, T = imu_next.shape[0], imu_next.shape[1]
        dev = imu_next.device
        mk = lambda: (torch.empty(B, T, 3, 3, device=dev), torch.empty(B, T, 3, device=dev))
        self.cur = [mk() for _ in self.stages]
        self.nxt = [mk() for _ in self.stages]
        for st, pose in zip(self.stages, self.cur):
            st.pose = pose
        self.pair = ConcurrentStages(self.stages, use_graph=False, unguarded=unguarded)
        self.pair.extra_nets = self.imus
        self.side = torch.cuda.Stream()
        self.sides = [self.side] + [torch.cuda.Stream() for _ in self.imus[1:]]
        self.side_by_side = True
        self.use_graph, self.graph = use_graph, None

    def _imu_forward(self, k, persistent=True):
        from . import blocks
        net, (Rn, tn) = self.imus[k], self.nxt[k]
        # (the stage bodies run beside these forwards: see blocks.two_chains; `persistent`: blocks.seq_xcd)
        with torch.no_grad(), blocks.two_chains(False), blocks.seq_xcd(persistent):
            R, t = net(self.imu_next)
            ops.copy2d(R.view(-1, 9), Rn.view(-1, 9))
            ops.copy2d(t.view(-1, 3), tn.view(-1, 3))

    def _imu_forwards(self):
        for k in reversed(range(len(self.imus))):             # (Lower's first, as in ConcurrentStages)
            self._imu_forward(k)

    def prime(self):
        """Head poses of the first minibatch (its IMU samples are in `imu_next`)."""
        self._imu_forwards()
        torch.cuda.synchronize()

    def _body(self):
        main = torch.cuda.current_stream()
        for (Rc, tc), (Rn, tn) in zip(self.cur, self.nxt):
            ops.copy2d(Rn.view(-1, 9), Rc.view(-1, 9))
            ops.copy2d(tn.view(-1, 3), tc.view(-1, 3))
        if self.pair.exclusive():
            # a net runs bf16 MFMAs: the prefetched forwards and the bodies as ONE chain (needs_exclusive)
            with ops.no_fork():
                self._imu_forwards()
            self.pair._bodies()                               # (forks only all-fp32 bodies, behind the forwards)
            return
        if self.side_by_side:
            # every forward that runs at once needs its own co-resident set of 256 workgroups for the persistent rnn_slow launch:
            # the device holds `slots` of them (2 on a whole MI355X); the others take the launch-per-timestep form
            slots = hip.lib().mmego_lstm_seq_xcd_slots()
            for n, k in enumerate(reversed(range(len(self.imus)))):
                self.sides[k].wait_stream(main)
                with torch.cuda.stream(self.sides[k]):
                    self._imu_forward(k, persistent=n < slots)
            self.pair._bodies()
            for sd in self.sides:
                main.wait_stream(sd)
            return
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side):
            self._imu_forwards()
        self.pair._bodies()
        main.wait_stream(self.side)

    def _mutable_state(self):
        # (a warm-up run also moves the prefetched head poses on: the `cur` / `nxt` buffers are put back with the stages' state)
        return super()._mutable_state() + [t for pr in (self.cur, self.nxt) for pose in pr for t in pose]
