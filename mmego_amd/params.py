"""Flat parameter / gradient / Adam-state storage for a module.

All parameters of a net live in ONE fp32 buffer (each tensor 16-byte aligned inside it) and every
nn.Parameter is re-pointed to a view of it; gradients live in a second flat buffer of the same layout.
That gives: one fused Adam launch per step, one RCCL all-reduce per step (reference has neither:
Processor/Train/Train_Upper.py:60,181-182 steps 54 tensors one by one), and float4-aligned weights for
the GEMM kernels.  state_dict keys/shapes are untouched, so shipped checkpoints load unchanged.
"""
import contextlib

import torch

from . import hip

ALIGN = 4  # floats


class FlatParams:
    def __init__(self, module):
        self.module = module
        self.params = [p for p in module.parameters()]
        # A module may ask for a layout of its own (``flat_param_order() -> list of its parameters``): tensors that one product
        # wants to treat as ONE matrix (the weights of two convolutions over the same input, stacked) then sit back to back in
        # the parameter AND gradient buffers.  state_dict keys and shapes are untouched; only the flat offsets move.
        order = getattr(module, "flat_param_order", None)
        if callable(order):
            wanted = list(order())
            if sorted(id(p) for p in wanted) != sorted(id(p) for p in self.params):
                raise ValueError("flat_param_order() must return every parameter of the module exactly once")
            self.params = wanted
        self.device = None
        self.flat_p = self.flat_g = None
        self.offsets = []
        self._gviews = {}
        self._counters = None

    def _layout(self):
        off = 0
        self.offsets = []
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        return off

    def ensure(self):
        """(Re)build the flat buffers if the module moved device or was re-materialised."""
        p0 = self.params[0]
        if (self.flat_p is not None and p0.device == self.device and
                p0.data_ptr() == self.flat_p.data_ptr() + 4 * self.offsets[0] and
                self.params[-1].data_ptr() == self.flat_p.data_ptr() + 4 * self.offsets[-1]):
            return self
        self.device = p0.device
        total = self._layout()
        flat_p = torch.zeros(total, dtype=torch.float32, device=self.device)
        flat_g = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._gviews = {}
        for p, off in zip(self.params, self.offsets):
            n = p.numel()
            flat_p[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat_p[off:off + n].view(p.shape)
            self._gviews[id(p)] = flat_g[off:off + n].view(p.shape)
        self.flat_p, self.flat_g = flat_p, flat_g
        # BatchNorm step counters: one int64 buffer, bumped with a single launch per training forward
        named = [(n, b) for n, b in self.module.named_buffers() if n.endswith("num_batches_tracked")]
        if named:
            flat_c = torch.stack([b.to(self.device).reshape(()) for _, b in named]).contiguous()
            for i, (name, _) in enumerate(named):
                owner_name, _, leaf = name.rpartition(".")
                self.module.get_submodule(owner_name)._buffers[leaf] = flat_c[i]
            self._counters = flat_c
        return self

    def grad(self, p):
        return self._gviews[id(p)]

    def rebind_grad(self, buf):
        """Move the flat gradient buffer into ``buf`` (1-D fp32, same length, 16-byte aligned): several nets' gradients can
        then live back to back in ONE buffer and be summed over the ranks by ONE collective (train_step.GradBucket).  Must
        happen before anything captures the old addresses (HIP graphs)."""
        self.ensure()
        if buf.numel() != self.flat_g.numel() or buf.dtype != torch.float32 or buf.device != self.flat_g.device or buf.data_ptr() % 16:
            raise ValueError("rebind_grad: need an aligned fp32 buffer of %d elements on %s" % (self.flat_g.numel(), self.flat_g.device))
        buf.copy_(self.flat_g)
        self.flat_g = buf
        for p, off in zip(self.params, self.offsets):
            self._gviews[id(p)] = buf[off:off + p.numel()].view(p.shape)
            if p.grad is not None:
                p.grad = self._gviews[id(p)]

    def tick_args(self, seed_ctr=None):
        """(counters, n, seed_ctr): the once-per-training-forward tick of a net -- BatchNorm num_batches_tracked += 1 for all
        layers and the next dropout seed -- as the arguments of the kernel that carries it (mmego_head_fk_forward; mmego_inc_i64
        is the same tick as a launch of its own)."""
        if self._counters is not None:
            return (self._counters, self._counters.numel(), seed_ctr)
        return (None, 0, seed_ctr)

    def bind_grads(self):
        """Expose the flat gradient views as ``p.grad`` (for torch optimisers / inspection)."""
        for p in self.params:
            if p.requires_grad:
                p.grad = self._gviews[id(p)]


class LrSchedule:
    """A learning-rate schedule over the optimiser's step count, evaluated inside the Adam launch (mmego_adam_step_sched; the header
    spells the multiplier out).  An immutable value: kind "constant" | "cosine" | "linear" | "step"; warmup W >= 0 steps of linear
    warm-up (step 1 at lr / W, step W the first at the full rate); span D >= 1, the steps a cosine or linear decay takes behind the
    warm-up; floor r in [0, 1), where the decay ends as a fraction of lr (step: its lower bound); every E >= 1 and gamma g in (0, 1]
    of the step decay.  Validation is the C side's.  `multiplier(t)` is the same arithmetic in Python floats, for what the host prints."""

    KINDS = ("constant", "cosine", "linear", "step")
    FIELDS = ("kind", "warmup", "span", "floor", "every", "gamma")

    def __init__(self, kind="constant", warmup=0, span=None, floor=0.0, every=None, gamma=None):
        def steps(name, val, least):
            try:
                ok = float(val) >= least and float(val) <= 2.0 ** 53 and float(val) == int(val)
            except (TypeError, ValueError, OverflowError):
                ok = False
            if not ok:
                raise ValueError("LrSchedule: %s has to be a whole number of steps >= %d, got %r" % (name, least, val))
            return int(val)
        if kind not in self.KINDS:
            raise ValueError("LrSchedule: kind has to be one of %s, got %r" % (", ".join(self.KINDS), kind))
        self.kind = kind
        self.warmup = steps("warmup", warmup, 0)
        try:
            self.floor = float(floor)
        except (TypeError, ValueError):
            self.floor = float("nan")
        if not 0.0 <= self.floor < 1.0:            # (false for NaN as well)
            raise ValueError("LrSchedule: floor has to lie in [0, 1), got %r" % (floor,))
        self.span = self.every = self.gamma = None
        if kind in ("cosine", "linear"):
            self.span = steps("span", span, 1)
        elif span is not None:
            raise ValueError("LrSchedule: span belongs to the cosine and linear kinds, not to %s" % kind)
        if kind == "step":
            self.every = steps("every", every, 1)
            try:
                self.gamma = float(gamma)
            except (TypeError, ValueError):
                self.gamma = float("nan")
            if not 0.0 < self.gamma <= 1.0:
                raise ValueError("LrSchedule: gamma has to lie in (0, 1], got %r" % (gamma,))
        elif every is not None or gamma is not None:
            raise ValueError("LrSchedule: every and gamma belong to the step kind, not to %s" % kind)

    def c_struct(self):
        """The MmegoLrSchedule of this schedule (a host struct; the entry point copies it into the kernel arguments)."""
        return hip.LrSchedule(kind=self.KINDS.index(self.kind), reserved=0, warmup=float(self.warmup), span=float(self.span or 0),
                              floor=self.floor, every=float(self.every or 0), gamma=float(self.gamma or 0.0))

    def multiplier(self, t):
        """lr_t / lr of step t >= 1, in float64."""
        import math
        t, W = float(t), float(self.warmup)
        w = t / W if W > 0 and t < W else 1.0
        s = t - W
        if not s > 0.0:
            return w
        if self.kind in ("cosine", "linear"):
            x = min(s, float(self.span)) / float(self.span)
            shape = (1.0 + math.cos(math.pi * x)) / 2.0 if self.kind == "cosine" else 1.0 - x
            return self.floor + (1.0 - self.floor) * shape
        if self.kind == "step":
            return max(self.floor, self.gamma ** math.floor(s / float(self.every)))
        return 1.0

    def to_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    @classmethod
    def from_dict(cls, d):
        if set(d) != set(cls.FIELDS):
            raise ValueError("LrSchedule.from_dict: expected the keys %s, got %s" % (", ".join(cls.FIELDS), ", ".join(sorted(map(str, d)))))
        return cls(**d)

    def __eq__(self, other):
        return isinstance(other, LrSchedule) and self.to_dict() == other.to_dict()

    def __hash__(self):
        return hash(tuple(self.to_dict().items()))

    def describe(self):
        """`<kind>, warm-up W steps, span D steps, floor r[, every E gamma g]` (the trainers' start line)."""
        text = "%s, warm-up %d steps, span %s steps, floor %g" % (self.kind, self.warmup, "-" if self.span is None else "%d" % self.span, self.floor)
        return text + (", every %d gamma %g" % (self.every, self.gamma) if self.kind == "step" else "")

    def __repr__(self):
        return "LrSchedule(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.FIELDS)


def lr_schedule_of(cfg, epochs, steps_per_epoch):
    """The LrSchedule a run's options ask for (--lr_schedule, --lr_warmup, --lr_min_ratio, --lr_decay_steps, --lr_step_every,
    --lr_step_gamma as config attributes); None where none is given.  A cosine or linear decay without --lr_decay_steps spans the rest
    of the run: epochs x steps_per_epoch (the optimiser steps of one epoch of THIS run) - warmup, at least 1."""
    kind, warmup = getattr(cfg, "lr_schedule", None), getattr(cfg, "lr_warmup", None)
    if kind is None and warmup is None:
        return None
    kind, warmup = kind or "constant", warmup or 0
    kw = {}
    if kind in ("cosine", "linear"):
        span = getattr(cfg, "lr_decay_steps", None)
        kw["span"] = max(1, int(epochs) * int(steps_per_epoch) - int(warmup)) if span is None else span
    if kind == "step":
        kw.update(every=getattr(cfg, "lr_step_every", None), gamma=getattr(cfg, "lr_step_gamma", None))
    return LrSchedule(kind, warmup=warmup, floor=getattr(cfg, "lr_min_ratio", None) or 0.0, **kw)


def decay_mask_words(layout, no_decay=()):
    """The decay mask of a flat buffer (mmego_adam_step_decay's ``decay_mask``) as a numpy uint64 array, on the host: one bit per float4,
    word w bit b covering float4 64 w + b, set where the element decays.  ``layout``: (name, offset, numel) triples in buffer order, as
    FusedAdam.layout() gives them -- every tensor starts on a float4 boundary (ALIGN) and owns its padding, so a float4 belongs to one
    tensor; ``no_decay``: the names whose tensors do not decay.  A name that is not in the layout is a ValueError.  ceil(n4 / 64) words;
    the bits beyond n4 in the last one are clear."""
    import numpy as np
    layout = [(str(n), int(o), int(k)) for n, o, k in layout]
    unknown = sorted(set(no_decay) - {n for n, _, _ in layout})
    if unknown:
        raise ValueError("no_decay names parameters this net does not have: %s" % ", ".join(unknown))
    spans = [(n, o, o + (k + ALIGN - 1) // ALIGN * ALIGN) for n, o, k in layout]
    if any(o % ALIGN for _, o, _ in spans):
        raise ValueError("decay_mask_words: every tensor has to start on a multiple of %d floats" % ALIGN)
    n4 = max([hi for _, _, hi in spans] + [0]) // ALIGN
    bits = np.ones(n4, dtype=np.uint8)
    skip = set(no_decay)
    for n, lo, hi in spans:
        if n in skip:
            bits[lo // ALIGN:hi // ALIGN] = 0
    padded = np.zeros((n4 + 63) // 64 * 64, dtype=np.uint8)
    padded[:n4] = bits
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def resolve_no_decay(module, no_decay):
    """FusedAdam's ``no_decay`` as a sorted tuple of parameter names: None -> (), "1d" -> every parameter with at most one dimension (biases,
    BatchNorm weight and bias, LSTM biases), an iterable of names -> those; a name the module does not have is a ValueError."""
    if no_decay is None:
        return ()
    named = list(module.named_parameters())
    if isinstance(no_decay, str):
        if no_decay != "1d":
            raise ValueError("no_decay has to be None, \"1d\" or an iterable of parameter names, got %r" % (no_decay,))
        return tuple(sorted(n for n, p in named if p.dim() <= 1))
    names = sorted({str(n) for n in no_decay})
    unknown = sorted(set(names) - {n for n, _ in named})
    if unknown:
        raise ValueError("no_decay names parameters this net does not have: %s" % ", ".join(unknown))
    return tuple(names)


def describe_decay(decoupled, no_decay):
    """`adamw|l2, all tensors decay | N tensors left out` (both sides of a refusal's message)."""
    return "%s, %s" % ("adamw (decoupled)" if decoupled else "l2 (coupled)",
                       "every tensor decays" if not no_decay else "no decay for %d tensors (%s%s)" % (
                           len(no_decay), ", ".join(no_decay[:3]), ", ..." if len(no_decay) > 3 else ""))


class FusedAdam:
    """torch.optim.Adam semantics (betas 0.9/0.999, eps 1e-8, coupled weight decay) in one launch.

    decoupled (False: the coupled L2 form above): torch.optim.AdamW's decay, p <- p - lr_t * weight_decay * p ahead of an update whose
    gradient carries no decay term, lr_t the rate of the step (the scheduled one under lr_schedule: the decay follows the schedule).
    no_decay (None: every tensor decays; "1d": every parameter with at most one dimension -- biases, BatchNorm weight and bias, LSTM
    biases; or an iterable of parameter names): tensors that are updated as with weight_decay = 0, in either form.  Both go through
    mmego_adam_step_decay (a bit mask over the flat buffer, built once on the host: decay_mask_words); an optimiser with neither makes
    exactly the calls below.  A state_dict carries them only where they are not the defaults.

    max_grad_norm (None: off): torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) ahead of every step, over THIS net's
    gradients, as two launches and no host read (mmego_grad_sqnorm, mmego_adam_step_clipped).  A step whose gradient norm is not
    finite is skipped on the device -- weights, moments and step count stay as they are -- and counted; `grad_stats()` reads the
    norms and counts seen since the last `reset_grad_stats()`.  float("inf") measures without ever clipping.

    ema_decay (None: off; else d in (0, 1)): an exponential moving average of the weights, `ema`, a second flat buffer in the layout
    of `flat_p`, updated by the step's own launch (mmego_adam_step_ema, mmego_adam_step_clipped_ema): ema <- ema + (1 - d)(p_new - ema)
    for every element the update touches.  DEFINITION: ema_0 is the weights as they are when the optimiser's buffers are built, which
    is its first use (step, state_dict, load_state_dict, averaged) -- for fine-tuning from a checkpoint, the checkpoint.  So there is
    no bias correction and no first step that differs; parameters that never train, and steps skipped as non-finite, keep ema equal to
    the weights.  Buffers of the module (BatchNorm running statistics) are not averaged: they are running averages already.
    `averaged()` evaluates with the average in place of the weights, `ema_state_dict()` is the module's state_dict with it.

    lr_schedule (None: off; else an LrSchedule): the rate of step t is lr * schedule.multiplier(t), computed by the step's own launch from
    the step count on the device (mmego_adam_step_sched, for all four forms above), so a captured graph replays another rate every step
    and a step skipped as non-finite consumes no schedule step.  `state` then has a fourth double, the rate of the last step taken
    (`current_lr()`).  Assigning `lr` between steps still changes nothing under a captured graph: the schedule is the way to move it."""

    STAT_KEYS = ("last", "sum", "max", "steps", "clipped", "skipped")

    def __init__(self, flat, lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, ema_decay=None,
                 lr_schedule=None, decoupled=False, no_decay=None):
        if lr_schedule is not None and not isinstance(lr_schedule, LrSchedule):
            raise ValueError("lr_schedule has to be a params.LrSchedule (or None: a constant rate), got %r" % (lr_schedule,))
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("max_grad_norm has to be > 0 (or None: no clipping), got %r" % (max_grad_norm,))
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:            # (false for NaN as well)
            raise ValueError("ema_decay has to lie in (0, 1) (or None: no weight average), got %r" % (ema_decay,))
        self.flat = flat
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.m = self.v = self.state = self._ticket = None
        self._skip = None
        self._part = self._stats = None
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema = None
        self._averaged = False            # inside averaged(): flat_p holds the average, ema the weights
        self.lr_schedule = lr_schedule
        self._sched = None if lr_schedule is None else lr_schedule.c_struct()      # (kept alive: a recorded launch holds the object)
        if decoupled not in (False, True, 0, 1):
            raise ValueError("decoupled has to be True (AdamW's decay) or False (the coupled L2 form), got %r" % (decoupled,))
        self.decoupled = bool(decoupled)
        self.no_decay = resolve_no_decay(flat.module, no_decay)      # (sorted names; (): every tensor decays)
        self._mask = None

    def _skip_ranges(self, f):
        """Element ranges of parameters that never receive a gradient (`module.never_trained()`, e.g. IMU_Net.fc3):
        torch.optim.Adam leaves a parameter with grad=None alone -- no moment update, no weight decay."""
        if self._skip is None:
            dead = {id(p) for p in getattr(f.module, "never_trained", lambda: ())()}
            spans = []
            for p, off in zip(f.params, f.offsets):
                if id(p) in dead:
                    end = off + (p.numel() + ALIGN - 1) // ALIGN * ALIGN
                    if spans and spans[-1][1] == off:
                        spans[-1][1] = end
                    else:
                        spans.append([off, end])
            if len(spans) > 4:
                raise ValueError("FusedAdam supports at most 4 disjoint never-trained parameter ranges")
            self._skip = torch.tensor([v for sp in spans for v in sp], dtype=torch.int64) if spans else False
        return self._skip

    def _ensure(self):
        f = self.flat.ensure()
        if self.m is None or self.m.device != f.device or self.m.numel() != f.flat_p.numel():
            self.m = torch.zeros_like(f.flat_p)
            self.v = torch.zeros_like(f.flat_p)
            self.state = torch.zeros(3 if self.lr_schedule is None else 4, dtype=torch.float64, device=f.device)
            self._ticket = torch.zeros(1, dtype=torch.int32, device=f.device)
            self._part = self._stats = None
            self.ema = None
            self._mask = None
        if self.no_decay and self._mask is None:
            # (one bit per float4, clear over the tensors that do not decay; built before the first step, so before anything captures its address)
            words = decay_mask_words(self._layout_of(f), self.no_decay)
            self._mask = torch.from_numpy(words.view("int64")).to(f.device)
        if self.ema_decay is not None and self.ema is None:
            # (ema_0 = the weights as they are now; built before the first step, so before anything captures its address)
            self.ema = f.flat_p.clone()
        if self.max_grad_norm is not None and self._part is None:
            # (only a clipping optimiser owns these; built before the first step, so before anything captures their addresses)
            self._part = torch.zeros(hip.lib().mmego_grad_norm_nblk(f.flat_p.numel()), dtype=torch.float64, device=f.device)
            self._stats = torch.zeros(8, dtype=torch.float64, device=f.device)
        return f

    def step(self):
        if self._averaged:
            raise RuntimeError("FusedAdam.step() inside averaged(): the parameters hold the average, not the weights to update")
        f = self._ensure()
        skip = self._skip_ranges(f)
        ranges = (skip if skip is not False else None, skip.numel() // 2 if skip is not False else 0)
        common = (f.flat_p, f.flat_g, self.m, self.v, f.flat_p.numel(), self.state, float(self.lr), float(self.betas[0]),
                  float(self.betas[1]), float(self.eps), float(self.weight_decay), *ranges, self._ticket)
        clip = avg = ()
        if self.max_grad_norm is not None:
            hip.call("grad_sqnorm", f.flat_g, f.flat_g.numel(), *ranges, self._part, self._part.numel())
            clip = (self._part, self._part.numel(), self.max_grad_norm, self._stats)
        if self.ema_decay is not None:
            avg = (self.ema, self.ema_decay)
        if self.decoupled or self._mask is not None:
            # (every option in one entry point; a NULL schedule is the unscheduled step, a NULL mask decays everything)
            hip.call("adam_step_decay", *common, *(clip or (None, 0, 0.0, None)), *(avg or (None, 0.0)), self._sched, self._mask,
                     int(self.decoupled))
        elif self.lr_schedule is not None:
            # (one entry point for the four forms: absent record buffers select the plain step, an absent average the step without one)
            hip.call("adam_step_sched", *common, *(clip or (None, 0, 0.0, None)), *(avg or (None, 0.0)), self._sched)
        else:
            # (an option's arguments stand behind the plain ones, under the name that says so)
            hip.call("adam_step" + ("_clipped" if clip else "") + ("_ema" if avg else ""), *common, *clip, *avg)
        # the update went through raw pointers (no tensor._version bump): tell the net to drop derived copies of its weights
        changed = getattr(f.module, "weights_changed", None)
        if changed is not None:
            changed()

    def current_lr(self):
        """The rate of the last step taken (one device read: state[3]); before the first step, the rate the first step will take.
        Without a schedule: lr."""
        if self.lr_schedule is None:
            return float(self.lr)
        self._ensure()
        t, _, _, rate = self.state.tolist()
        return rate if t > 0 and rate > 0 else float(self.lr) * self.lr_schedule.multiplier(t + 1)

    def zero_grad(self):
        pass  # every backward overwrites the flat gradient buffer

    def _exchange(self, f):
        """Exchange the CONTENTS of flat_p and ema (HIP graphs and the nets' parameter views hold the addresses) and have the net drop
        what it derived from the old contents."""
        keep = f.flat_p.clone()
        f.flat_p.copy_(self.ema)
        self.ema.copy_(keep)
        changed = getattr(f.module, "weights_changed", None)
        if changed is not None:
            changed()

    @contextlib.contextmanager
    def averaged(self):
        """Inside the context the module runs on the averaged weights; on exit the weights are back bit for bit (an exchange, no
        arithmetic).  Not re-entrant, and no step() inside."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdam.averaged(): this optimiser keeps no weight average (ema_decay=None)")
        if self._averaged:
            raise RuntimeError("FusedAdam.averaged() is not re-entrant: the parameters already hold the average")
        f = self._ensure()
        self._exchange(f)
        self._averaged = True
        try:
            yield self
        finally:
            self._exchange(f)
            self._averaged = False

    def ema_state_dict(self):
        """The module's state_dict() with every parameter taken from the average (copies).  Buffers -- BatchNorm running statistics and
        step counters -- are the live ones: they are not averaged."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdam.ema_state_dict(): this optimiser keeps no weight average (ema_decay=None)")
        f = self._ensure()
        src = f.flat_p if self._averaged else self.ema
        sd = f.module.state_dict()
        shapes = {n: p.shape for n, p in f.module.named_parameters()}
        for name, off, k in self.layout():
            sd[name] = src[off:off + k].view(shapes[name]).clone()
        return sd

    def grad_stats(self):
        """The gradient norms of the steps since the last reset, from ONE device read: {"last", "sum", "max", "steps", "clipped",
        "skipped", "mean"} (mean and max over the steps with a finite norm).  None without max_grad_norm."""
        if self.max_grad_norm is None:
            return None
        self._ensure()
        vals = self._stats.tolist()
        out = dict(zip(self.STAT_KEYS, vals))
        for k in ("steps", "clipped", "skipped"):
            out[k] = int(out[k])
        finite = out["steps"] - out["skipped"]
        out["mean"] = out["sum"] / finite if finite else float("nan")
        return out

    def reset_grad_stats(self):
        if self.max_grad_norm is not None:
            self._ensure()
            self._stats.zero_()

    def layout(self):
        """The fingerprint of the flat layout: (parameter name, offset, numel) in buffer order.  The order inside the flat buffers
        is the net's own business (`flat_param_order`) and has changed between rounds, so a saved optimizer state carries it."""
        return self._layout_of(self._ensure())

    @staticmethod
    def _layout_of(f):
        names = {id(p): n for n, p in f.module.named_parameters()}
        return [(names[id(p)], int(off), int(p.numel())) for p, off in zip(f.params, f.offsets)]

    def decay_counts(self):
        """(tensors, elements) that weight decay reaches: everything but the no_decay tensors and those that never train."""
        f = self._ensure()
        dead = {id(p) for p in getattr(f.module, "never_trained", lambda: ())()}
        left = [p for n, p in f.module.named_parameters() if n not in set(self.no_decay) and id(p) not in dead]
        return len(left), sum(p.numel() for p in left)

    def state_dict(self):
        """Moments and step counters (host copies) + hyper-parameters + the layout the moments are stored in: everything a
        bit-exact resume needs, also after the flat layout of the net has changed."""
        if self._averaged:
            raise RuntimeError("FusedAdam.state_dict() inside averaged(): weights and average are exchanged")
        self._ensure()
        sd = {"m": self.m.cpu(), "v": self.v.cpu(), "state": self.state.cpu(), "lr": self.lr, "betas": tuple(self.betas),
              "eps": self.eps, "weight_decay": self.weight_decay, "layout": self.layout(), "max_grad_norm": self.max_grad_norm}
        if self.ema_decay is not None:     # (an optimiser without an average writes the state it always wrote)
            sd["ema"], sd["ema_decay"] = self.ema.cpu(), self.ema_decay
        if self.lr_schedule is not None:
            sd["lr_schedule"] = self.lr_schedule.to_dict()
        if self.decoupled:                 # (likewise: only what is not the default)
            sd["decoupled"] = True
        if self.no_decay:
            sd["no_decay"] = list(self.no_decay)
        return sd

    def load_state_dict(self, sd):
        """Moments are matched to parameters BY NAME through the saved layout; a state saved under another flat order lands on
        the right parameters.  A state without a layout (written before r03) is only accepted where no ambiguity exists: the net
        has no layout of its own (registration order then and now).  Anything else is refused -- equal element counts say
        nothing about where a parameter's moments are."""
        if self._averaged:
            raise RuntimeError("FusedAdam.load_state_dict() inside averaged(): weights and average are exchanged")
        if sd.get("lr_schedule") is not None:
            theirs = LrSchedule.from_dict(sd["lr_schedule"])
            if theirs != self.lr_schedule:
                raise ValueError("optimizer state was saved under the learning-rate schedule %r, this optimiser was built with %r: "
                                 "build it with the saved one" % (theirs, self.lr_schedule))
        elif sd["state"].numel() != 3:
            raise ValueError("optimizer state has %d state words and names no learning-rate schedule" % sd["state"].numel())
        theirs = (bool(sd.get("decoupled", False)), tuple(sorted(str(n) for n in (sd.get("no_decay") or ()))))
        if (self.decoupled, self.no_decay) not in ((False, ()), theirs):
            raise ValueError("optimizer state was saved under the weight decay [%s], this optimiser was built with [%s]: build it with "
                             "the saved one, or with neither option" % (describe_decay(*theirs), describe_decay(self.decoupled, self.no_decay)))
        f = self._ensure()
        cur = self.layout()
        saved = sd.get("layout")
        if saved is None:
            reg, off = [], 0
            names = {id(p): n for n, p in f.module.named_parameters()}
            for p in f.module.parameters():
                reg.append((names[id(p)], off, p.numel()))
                off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
            if reg != cur or sd["m"].numel() != f.flat_p.numel():
                raise ValueError("optimizer state carries no layout fingerprint and this net orders its flat buffer itself "
                                 "(flat_param_order): the saved Adam moments cannot be matched to parameters; re-save the "
                                 "training state with this build or resume from the model weights alone")
            saved = cur
        saved = [(str(n), int(o), int(k)) for n, o, k in saved]
        if sorted((n, k) for n, _, k in saved) != sorted((n, k) for n, _, k in cur):
            missing = sorted({n for n, _, _ in cur} ^ {n for n, _, _ in saved})
            raise ValueError("optimizer state belongs to another net: parameters differ (%s%s)" %
                             (", ".join(missing[:4]) or "shapes", " ..." if len(missing) > 4 else ""))
        if sd.get("ema_decay") is not None:     # (as max_grad_norm: the saved value wins, and a state with an average switches averaging on)
            self.ema_decay = float(sd["ema_decay"])
            self._ensure()                      # (the average's buffer, should the state switch averaging on)
        carried = [("m", self.m), ("v", self.v)] + ([("ema", self.ema)] if sd.get("ema_decay") is not None else [])
        if saved == cur and sd["m"].numel() == f.flat_p.numel():
            for key, dst in carried:
                dst.copy_(sd[key])
        else:
            where = {n: o for n, o, _ in saved}
            for key, dst in carried:
                new = torch.zeros(f.flat_p.numel())
                for n, o, k in cur:
                    so = where[n]
                    new[o:o + k] = sd[key][so:so + k]
                dst.copy_(new)
        if (self.decoupled, self.no_decay) != theirs:      # (as lr and ema_decay: the saved values win; a state without the keys is coupled, all-decay)
            self.decoupled, self.no_decay = theirs[0], resolve_no_decay(f.module, theirs[1])
            self._mask = None
            self._ensure()
        if self.ema_decay is not None and sd.get("ema_decay") is None:
            self.ema.copy_(f.flat_p)
            print("[mmego_amd] optimizer state carries no weight average: the average (decay %g) restarts from the loaded weights" % self.ema_decay)
        # (a three-word state into a scheduled optimiser: the schedule takes up at the saved step count; state[3] is 0 until its first step)
        self.state.zero_()
        self.state[:sd["state"].numel()].copy_(sd["state"])
        self.lr, self.betas, self.eps, self.weight_decay = sd["lr"], tuple(sd["betas"]), sd["eps"], sd["weight_decay"]
        if "max_grad_norm" in sd:          # (as lr: the saved value wins, a resumed run clips as the run it continues; a state from
            self.max_grad_norm = None if sd["max_grad_norm"] is None else float(sd["max_grad_norm"])    # before the key: ours stays)
            self._ensure()                 # (the record buffer, should the state switch clipping on)
