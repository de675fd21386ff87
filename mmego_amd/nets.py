"""IMUNet / UpperNet / LowerNet on the MI355X HIP path.

Drop-in surface: class names, constructor and forward signatures, return tuples and state_dict
keys/shapes of the reference's Net/IMU_Net.py:50-94, Net/Upper_Net.py:367-388 and
Net/Lower_Net.py:170-239 (checked against the shipped checkpoints in tests/).  The sub-modules are
parameter containers only (their initialisation order matches the reference, so torch.manual_seed gives
the same weights); every forward/backward below is a hand-written sequence of HIP kernels from
libmmego_hip.so.  There is no CPU path: calling a net on a CPU tensor raises.

Reference quirks reproduced: Q1 in-place head transform of the caller's `x`,
Q2 body row n % B, Q4 FK walk order, Q6 degenerate fusion gate, Q7 unused fc3 / ignored h0 arguments,
Q8 re-view (not permute) of the ST-GCN output.
"""
import os
import time

import torch
import torch.nn as nn

from . import blocks, hip, ops
from .blocks import LstmParams
from .params import FlatParams
from .skeleton import JOINTS_UPPER, LOWER_POINTS, gcn_adjacency


_FUSED_FRONT = True      # eval-mode Upper_Net front end as one launch (front.hip)
_GCN_FUSED = True          # training: the ST-GCN's fused block kernels (gcn_fused.hip)
_FUSED_HEAD_LOSS = True    # training: kinematics + loss + its backward as one launch (mmego_head_fk_loss)
_BF16_FUSED_FC1 = True     # bf16 mode: fc1 written straight as the fused step's fragment-major operand
# (the four flags above are not user settings: the forms they switch off are what shapes outside the fused kernels' ranges run, and the
#  tests flip them to hold the fused kernels to those forms bit for bit)


def _require_gpu(t, who):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError("%s runs on the MI355X HIP path only (got a %s tensor); there is no CPU fallback"
                           % (who, getattr(t, "device", type(t))))
    hip.lib()


def _f32c(t):
    return t.contiguous() if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


class _NetBase(nn.Module):
    """Shared plumbing: flat parameters, arenas, autograd bridge, save/load."""

    def __init__(self):
        super().__init__()
        self._flat = None
        self._arenas = {}
        self._seed = None
        self.lstm_dropout = None      # None -> use the LstmParams.dropout value in training mode
        # "fp32" (default, the parity path) or "bf16": EVAL forwards run their dense products with bf16 operands and fp32
        # accumulation where a kernel for it exists (BASELINE config 5; training always runs fp32)
        self.precision = os.environ.get("MMEGO_EVAL_PRECISION", "fp32")

    # -- derived weight copies ----------------------------------------------------------------------
    # Re-laid-out / folded copies of parameters and BatchNorm statistics (eval-mode packs: _tconv_packed, _gcn_bf16_pack, the bf16
    # LSTM weights of IMUNet) are keyed on (tensor._version, data_ptr) -- but the fused Adam and the train-mode BatchNorm kernels
    # write through raw pointers, which never bumps _version.  So the copies are dropped whenever the weights MAY
    # change: on .train() and on every params.FusedAdam.step() of this net; the next eval forward packs again.
    _derived = ("_tconv_packed", "_gcn_bf16_pack")

    def weights_changed(self):
        for name in self._derived:
            self.__dict__.pop(name, None)

    def train(self, mode=True):
        if mode:
            self.weights_changed()
        return super().train(mode)

    def _bf16_eval(self, training):
        if self.precision not in ("fp32", "bf16"):
            raise ValueError("%s.precision must be 'fp32' or 'bf16', got %r" % (type(self).__name__, self.precision))
        return self.precision == "bf16" and not training

    # -- storage -------------------------------------------------------------------------------
    def flat(self):
        if self._flat is None:
            self._flat = FlatParams(self)
        return self._flat.ensure()

    def arena(self, name):
        dev = next(self.parameters()).device
        ar = self._arenas.get(name)
        if ar is None or ar.device != dev:
            ar = ops.Arena(dev)
            self._arenas[name] = ar
        return ar

    def _pulled_pairs(self):
        """{name: name of the parameter to lay out directly behind it} -- see flat_param_order."""
        pulled = {}
        for mname, m in self.named_modules():
            if isinstance(m, LstmParams) and m.hidden_size == 64 and m.num_directions == 2:
                # BiLSTM(64) stacks: the two directions' input weights of a layer back to back, so that the layer's input
                # gradient is ONE product dgates[rows, 512] . [W_ih ; W_ih_reverse] (blocks.lstm64_backward)
                # ... and the directions' bias_ih / bias_hh pairs, so that the bias gradients (row sums of the gate gradients) come
                # out of the two batched weight-gradient products as their `asum` (no column-sum launch)
                for l in range(m.num_layers):
                    for kind in ("weight_ih", "bias_ih", "bias_hh"):
                        pulled["%s.%s_l%d" % (mname, kind, l)] = "%s.%s_l%d_reverse" % (mname, kind, l)
        return pulled

    def flat_param_order(self):
        """Flat-buffer layout (params.FlatParams): registration order, except that tensors which one product treats as a single
        stacked matrix follow each other (`_pulled_pairs`; ops.stacked builds the view).  state_dict keys are untouched."""
        named = list(self.named_parameters())
        pulled = self._pulled_pairs()
        by_name = dict(named)
        late = set(pulled.values())
        out = []
        for name, prm in named:
            if name in late:
                continue
            out.append(prm)
            if name in pulled:
                out.append(by_name[pulled[name]])
        return out

    def seed_counter(self):
        dev = next(self.parameters()).device
        if self._seed is None or self._seed.device != dev:
            self._seed = torch.tensor([0x9E3779B97F4A7C15 & 0x7FFFFFFFFFFFFFFF], dtype=torch.int64, device=dev)
        return self._seed

    def _ptr_table(self, slot, tensors):
        """Host-side int64 table of ``tensors``' device pointers (one kernel argument for all of them), kept under ``slot`` and rebuilt
        when a tensor moved."""
        ptrs = tuple(v.data_ptr() for v in tensors)
        ent = self.__dict__.get(slot)
        if ent is None or ent[0] != ptrs:
            ent = self.__dict__[slot] = (ptrs, torch.tensor(ptrs, dtype=torch.int64))
        return ent[1]

    def _bridged(self, args):
        """End of a public forward whose inputs want no gradient: through the autograd node when a parameter may want one, else the plain
        pipeline that keeps nothing."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            self.flat()
            return _Bridge.apply(self, 1, args, *self._flat.params)
        return self._forward_impl(*args, stash=False)

    # -- kinematics head, optionally with the trainer's loss and the start of backward in the same launch ----------------
    loss_hook = None      # (target [B,T,21,3], joint map int32, loss buffer [2], scale): set by train_step.StageStep around a step

    def _head_fk(self, ar, which, y, body, B, F, q, jh, R, t, l, tick, stash, pose=None):
        """mmego_head_fk_forward; with a loss hook (training step, <= 512 frames) mmego_head_fk_loss instead: kinematics, head-to-world
        transform, L1(sum) loss, its gradient and the kinematics' backward in one launch -- dy lands in the arena and
        _backward_impl skips its first launch (bit-identical to the three separate launches).
        pose = (dRw, dtw) (a differentiable head pose): the fused launch leaves the world transform's pose gradients there as well."""
        hook = self.loss_hook
        self._dy_ready = False
        if hook is not None and stash and _FUSED_HEAD_LOSS:
            target, jmap, loss2, scale = hook
            dy = ar.get("dy", (F, y.shape[1]))
            nb = (F + 63) // 64
            fresh = not ar.has("fkloss.scratch%d" % nb)
            scr = ar.get("fkloss.scratch%d" % nb, (2 * nb + 1,), dtype=torch.float64)
            if fresh:
                scr.zero_()          # (the ticket starts at 0; every launch leaves it 0.  One-time, outside any captured graph: warm-up)
            if pose is not None:
                hip.call("head_fk_loss_pose", which, y, body, B, F, q, jh, R, t, l, *tick, target, jmap, target.shape[-2], float(scale), loss2,
                         dy, scr, *pose)
            else:
                hip.call("head_fk_loss", which, y, body, B, F, q, jh, R, t, l, *tick, target, jmap, target.shape[-2], float(scale), loss2, dy, scr)
            self._dy_ready = True
        else:
            hip.call("head_fk_forward", which, y, body, B, F, q, jh, R, t, l, *tick)

    def _head_fk_backward(self, ar, which, y, body, B, F, dl, dy, R, jh_shape, pose, second=False):
        """Start of every backward, _head_fk's companion: the kinematics' backward dl -> dy (world -> head frame inside the kernel) -- unless
        the fused loss launch has left dy already.  pose = (dR, dt): ... and the world transform's share of the head pose's gradients
        (which that launch has left as well).  second: a gradient of its own BEHIND the fused launch's, so launched all the same."""
        if getattr(self, "_dy_ready", False) and not second:
            return
        if pose is not None:
            hip.call("head_fk_backward_pose", which, y, body, B, F, dl, dy, R, ar.get("jh", jh_shape), *pose)
        else:
            hip.call("head_fk_backward", which, y, body, B, F, dl, dy, R)

    # -- head-pose gradients of the Upper nets (UpperNet, nets_local.UpperNetwlocal): the head-frame transform in front ----------------
    _pose = None          # (raw, t, dR, dt) behind a pose_grad forward: the untransformed points, the translation, the gradients' arena buffers

    def pose_grads(self):
        """(dR [F,3,3], dt [F,3]) of the last backward behind a pose_grad forward: arena buffers, rewritten by the next one."""
        if getattr(self, "_pose", None) is None:
            raise RuntimeError("%s.pose_grads: the last forward did not ask for the head pose's gradients" % type(self).__name__)
        return self._pose[2], self._pose[3]

    def _pose_begin(self, ar, x, x_src, t, pose_grad, stash):
        """Start of a forward that transforms x [B,T,N,Cx] into the head frame in place: without pose_grad nothing is kept and nothing
        launched.  With it: the UNTRANSFORMED points (x_src when given -- the caller leaves it alone until backward has run -- else a copy
        taken here, ahead of the transform) and the arena buffers dR, dt that _backward_impl fills."""
        self._pose = None
        if not pose_grad:
            return
        if not stash:
            raise ValueError("%s: pose_grad needs a forward that keeps its activations (stash=True)" % type(self).__name__)
        B, T, N, Cx = x.shape
        F, rows = B * T, B * T * N
        if x_src is not None:
            raw = x_src.view(rows, Cx)
        else:
            raw = ar.get("pts_raw", (rows, Cx))
            ops.copy2d(x.view(rows, Cx), raw)
        self._pose = (raw, t, ar.get("dR", (F, 3, 3)), ar.get("dt", (F, 3)))

    def _pose_head_share(self, F, N, R, dfeats, dpts):
        """End of such a net's backward behind a pose_grad forward (nothing otherwise): the head-frame transform's share of dR, dt, ADDED
        to the world transform's (which the kinematics launch has left in the buffers).  The transformed xyz feed PointNet's first layer (dpts) and the first columns of the per-point
        feature rows (dfeats: GlobalPointNet's input and, in UpperNetwlocal, the grouped rows' offsets xyz - anchor, whose gradient the
        anchor scatter has added there); range, velocity and intensity do not depend on the pose."""
        if self._pose is None:
            return
        raw, t, dR, dt = self._pose
        hip.call("transform2h_backward", raw, raw.stride(0), F, N, R, t, dfeats, dfeats.stride(0), dpts, dpts.stride(0), 1, dR, dt)

    def _drop_p(self, lstm):
        if not self.training:
            return 0.0
        return float(lstm.dropout if self.lstm_dropout is None else self.lstm_dropout)

    # -- checkpoint I/O (reference Net/*.py save/load; map_location handled correctly) ----------
    def save(self, name=None):
        if name is None:
            name = time.strftime("checkpoints/%m%d_%H_%M_%S.pth")
        torch.save(self.state_dict(), name)
        return name

    def load(self, pathname):
        dev = next(self.parameters()).device
        self.load_state_dict(torch.load(pathname, map_location=dev))


def _bridge_backward(ctx, dl):
    """What every bridge's backward starts with: the net's backward pipeline on d loss / d (first output), gradients bound to .grad."""
    if not ctx.net.training:
        raise NotImplementedError("backward through an eval-mode net (running-stat BatchNorm) is not supported; "
                                  "the reference detaches frozen nets (Train_Lower.py:195-196)")
    ctx.net._backward_impl(dl)
    ctx.net.flat().bind_grads()


def _grads_for_caller(ctx, first, grads, like):
    """Input gradients as autograd takes them: ``grads`` belong to the forward arguments from position ``first`` on, ``like`` holds their
    (shape, dtype); only those somebody needs, as copies (the arena's buffers are rewritten by the next step, and autograd may keep
    what it is handed as .grad)."""
    return tuple(g.clone().view(shape).to(dtype) if (ctx.needs_input_grad[first + i] and g is not None) else None
                 for i, (g, (shape, dtype)) in enumerate(zip(grads, like)))


class _Bridge(torch.autograd.Function):
    """One autograd node per net: forward/backward are the hand-written kernel pipelines."""

    @staticmethod
    def forward(ctx, net, nout, args, *params):
        ctx.net = net
        outs = net._forward_impl(*args)
        ctx.mark_non_differentiable(*outs[nout:])
        return outs

    @staticmethod
    def backward(ctx, *grads):
        _bridge_backward(ctx, grads[0])
        return (None, None, None) + (None,) * len(ctx.net._flat.params)


def _pose_wants_grad(*ts):
    return torch.is_grad_enabled() and any(isinstance(v, torch.Tensor) and v.requires_grad for v in ts)


def _refuse_pose_grad(who, **named):
    """Nets whose backward owes its inputs nothing yet: a differentiable input must not lose its gradient silently."""
    bad = [k for k, v in named.items() if isinstance(v, torch.Tensor) and v.requires_grad]
    if bad and torch.is_grad_enabled():
        raise NotImplementedError("%s: %s require%s grad, but this net's backward produces no input gradients (UpperNet differentiates "
                                  "its head pose R, t; LowerNet its upper_l, R, t and UpperNetwlocal its R, t once "
                                  "differentiable_inputs = True); detach them"
                                  % (who, ", ".join(bad), "s" if len(bad) == 1 else ""))


class _PoseBridge(torch.autograd.Function):
    """_Bridge of UpperNet (and of UpperNetwlocal with differentiable_inputs) with the head pose as differentiable inputs: backward returns
    dR, dt beside the parameter gradients.  ``args``: the forward's arguments in front of R, t."""

    @staticmethod
    def forward(ctx, net, args, R, t, *params):
        ctx.net = net
        outs = net._forward_impl(*args, R, t, pose_grad=True)
        ctx.mark_non_differentiable(*outs[1:])
        ctx.like = [(v.shape, v.dtype) for v in (R, t)]
        return outs

    @staticmethod
    def backward(ctx, *grads):
        _bridge_backward(ctx, grads[0])
        return (None, None) + _grads_for_caller(ctx, 2, ctx.net.pose_grads(), ctx.like) + (None,) * len(ctx.net._flat.params)


class _InputBridge(torch.autograd.Function):
    """_Bridge of LowerNet (differentiable_inputs) with upper_l, R, t as differentiable inputs: backward returns their gradients beside
    the parameter gradients -- only those somebody needs."""

    @staticmethod
    def forward(ctx, net, args, upper_l, R, t, *params):
        ctx.net = net
        x, body, pin = args
        need = ctx.needs_input_grad
        want = (("upper_l",) if need[2] else ()) + (("pose",) if (need[3] or need[4]) else ())
        outs = net._forward_impl(upper_l, x, body, R, t, pin, input_grad=want)
        ctx.mark_non_differentiable(*outs[1:])
        ctx.like = [(v.shape, v.dtype) for v in (upper_l, R, t)]
        return outs

    @staticmethod
    def backward(ctx, *grads):
        _bridge_backward(ctx, grads[0])
        return (None, None) + _grads_for_caller(ctx, 2, ctx.net.input_grads(), ctx.like) + (None,) * len(ctx.net._flat.params)


# =====================================================================================================
# Upper_Net
# =====================================================================================================
class _Mlp3(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.conv1 = nn.Conv1d(dims[0], dims[1], 1)
        self.cb1 = nn.BatchNorm1d(dims[1])
        self.conv2 = nn.Conv1d(dims[1], dims[2], 1)
        self.cb2 = nn.BatchNorm1d(dims[2])
        self.conv3 = nn.Conv1d(dims[2], dims[3], 1)
        self.cb3 = nn.BatchNorm1d(dims[3])


class PointNet(_Mlp3):
    def __init__(self):
        super().__init__((6, 8, 16, 24))


class GlobalPointNet(_Mlp3):
    def __init__(self):
        super().__init__((28, 32, 48, 64))
        self.attn = nn.Linear(64, 1)


class GlobalModule(nn.Module):
    def __init__(self):
        super().__init__()
        self.gpointnet = GlobalPointNet()
        self.grnn = LstmParams(64, 64, 3, dropout=0.1, bidirectional=True)


class MLPHead(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = nn.Linear(128, 128)
        self.fc2 = nn.Linear(128, 14 * 6 + 3)


class _UpperBase(_NetBase):
    """The spine of both Upper nets (UpperNet below, nets_local.UpperNetwlocal): PointNet and the global branch in front -- checked,
    transformed into the head frame, stashed --, the two-layer head with the kinematics behind whatever sequence model(s) the net has,
    and the same three pieces backward.  The nets keep their sequence models, their `_saved`, the anchor branch and the ORDER of their
    backward's launches: the pieces below defer nothing and open no dw_reduce_group themselves."""

    state_pairs = 1       # (h0, c0) pairs in the forward's signature: train_step.call_upper hands one zero pair to each

    def __init__(self):
        super().__init__()
        self.module0 = PointNet()                 # (these two first: the subclasses' modules register behind them -- state_dict keys, flat layout)
        self.module1 = GlobalModule()

    def _front_one_launch(self, x, x_src, R, t, vec, attn):
        """A net's own form of the whole front as one launch, when it has one for this call: True when it ran."""
        return False

    def _front(self, ar, x, x_src, R, t, stash, pose_grad):
        """x [B,T,N,Cx] into the head frame in place (Q1), PointNet, GlobalPointNet, attention pooling over the points.
        x_src (optional, x's shape): the minibatch is read from there and x receives the transformed copy (one launch for a trainer's
        'fresh batch' copy and the transform).  pose_grad: see _pose_begin.
        -> (feats [rows,28] -- None behind _front_one_launch --, vec [F,64], attention weights [F,N,1], R, t as contiguous fp32)."""
        who = type(self).__name__
        if not (x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("%s: x must be a contiguous fp32 tensor (it is transformed in place)" % who)
        if x_src is not None and not (x_src.dtype == torch.float32 and x_src.is_contiguous() and x_src.shape == x.shape):
            raise ValueError("%s: x_src must be a contiguous fp32 tensor of x's shape" % who)
        training = self.training
        B, T, N, Cx = x.shape
        F, rows = B * T, B * T * N
        R, t = _f32c(R), _f32c(t)
        vec = ar.get("vec", (F, 64))
        attn = torch.empty((F, N, 1), dtype=torch.float32, device=x.device)
        self._pose_begin(ar, x, x_src, t, pose_grad, stash)
        if not stash and self._front_one_launch(x, x_src, R, t, vec, attn):
            return None, vec, attn, R, t          # (feats, pts, g3 are not taken from the arena)
        feats = ar.get("feats", (rows, 28))
        keep = ar.get("pts", (rows, Cx)) if stash else None
        if Cx <= 8:
            # Q1: in place on the caller's tensor; the copy kept for backward and the xyz + intensity columns of the feature buffer
            # leave from the same launch, and a trainer's fresh minibatch (x_src) enters through it
            ops.transform2h_(x, R, t, src=x_src, keep=keep, feats=feats, nfeat=4)
            pts = keep if stash else x.view(rows, Cx)
        else:
            if x_src is not None:
                ops.copy2d(x_src.view(rows, Cx), x.view(rows, Cx))
            ops.transform2h_(x, R, t)
            pts = x.view(rows, Cx)
            if stash:
                ops.copy2d(pts, keep)
                pts = keep
            ops.copy2d(pts[:, :4], feats[:, :4])
        blocks.mlp3_forward(ar, "m0", self.module0, pts, feats[:, 4:28], training)
        g3 = ar.get("g3", (rows, 64))
        gpn = self.module1.gpointnet
        self._gpool_fused = bool(stash and blocks.pool128_fusable(gpn, feats, N, training))
        if self._gpool_fused:       # the pooling inside the chain's last launch: g3 (the activated rows) is never stored
            blocks.mlp3_forward(ar, "gp", gpn, feats, g3, training, pool=(gpn.attn, vec, attn))
        else:
            blocks.mlp3_forward(ar, "gp", gpn, feats, g3, training)
            blocks.attn_pool_forward(g3, gpn.attn, F, N, 64, vec, attn)
        return feats, vec, attn, R, t

    def _head(self, ar, fc1, fc2, inp, body, B, T, R, t, stash):
        """fc1 + ReLU, fc2, then kinematics + head-to-world transform (+ loss, + the world transform's share of dR, dt) as one launch
        (Net/Upper_Net.py:393-404) -> (l [B,T,15,3], q [B,T,14,3,3])."""
        F = B * T
        h1 = ar.get("h1", (F, 128))
        ops.linear(inp, fc1.weight, fc1.bias, h1, relu=True)
        y = ar.get("y", (F, 87))
        ops.linear(h1, fc2.weight, fc2.bias, y)
        q = torch.empty((B, T, 14, 3, 3), dtype=torch.float32, device=inp.device)
        jh = ar.get("jh", (F, 15, 3))
        l = torch.empty((B, T, 15, 3), dtype=torch.float32, device=inp.device)
        tick = self._flat.tick_args(self.seed_counter()) if self.training else (None, 0, None)   # BatchNorm counters + dropout seed
        pose = self._pose
        self._head_fk(ar, 0, y, body, B, F, q, jh, R, t, l, tick, stash, pose=pose[2:] if pose is not None else None)
        return l, q

    def _head_backward(self, ar, fc1, fc2, inp, dinp, F, G, leaves=None):
        """dy -> d ``inp`` through fc2, the ReLU and fc1; the weight gradients at once or, with ``leaves``, when the caller runs those."""
        dh1 = ar.get("dh1", (F, 128))
        blocks.linear_backward(ar.get("dy", (F, 87)), ar.get("h1", (F, 128)), fc2, G, dh1, relu_input=True, leaves=leaves)
        blocks.linear_backward(dh1, inp, fc1, G, dinp, leaves=leaves)

    def _global_backward(self, ar, F, N, attn, dvec, G):
        """The global branch behind d vec: attention pooling and GlobalPointNet, inside the pooled chain's launches or as the launch
        chain, whichever the forward ran -> d feats [rows,28]."""
        rows = F * N
        g3, dg3 = ar.get("g3", (rows, 64)), ar.get("dg3", (rows, 64))
        feats = ar.get("feats", (rows, 28))
        gpn = self.module1.gpointnet
        if getattr(self, "_gpool_fused", False):
            blocks.pool128_backward_fused(ar, "gp", gpn, gpn.attn, attn, ar.get("vec", (F, 64)), dvec, rows, dg3, G)
            return blocks._mlp3_backward_fused(ar, "gp", gpn, feats, dg3, G, True, have_sums=True)
        blocks.attn_pool_backward(ar, "gpool", g3, gpn.attn, attn, dvec, F, N, 64, dg3, G)
        return blocks.mlp3_backward(ar, "gp", gpn, feats, g3, dg3, G, True)

    def _pointnet_backward(self, ar, F, N, dfeats, G):
        """PointNet behind its columns of d feats -> d pts, formed only for a differentiable head pose (_pose_head_share takes it, behind
        the caller's dw_reduce_group)."""
        rows = F * N
        feats = ar.get("feats", (rows, 28))
        return blocks.mlp3_backward(ar, "m0", self.module0, ar.get("pts", (rows, 6)), feats[:, 4:28], dfeats[:, 4:28], G, self._pose is not None)


class UpperNet(_UpperBase):
    """forward(x[B,T,N,6], h0_g[6,B,64], c0_g[6,B,64], initial_body[B,20,3], R[B,T,3,3], t[B,T,3])
    -> (l[B,T,15,3], q[B,T,14,3,3], global_weights[B*T,N,1], hn_g, cn_g).  MUTATES x (Q1).
    R, t that require grad receive their gradients from backward (both transforms: head frame in front, world frame behind);
    x, initial_body, h0_g, c0_g are not differentiable."""

    def __init__(self):
        super().__init__()
        self.mlpHead = MLPHead()

    def forward(self, x, h0_g, c0_g, initial_body, R, t):
        _require_gpu(x, "UpperNet")
        args = (x, h0_g, c0_g, initial_body, R, t)
        if _pose_wants_grad(R, t):
            self.flat()
            return _PoseBridge.apply(self, args[:4], R, t, *self._flat.params)
        return self._bridged(args)

    # -- pipelines ---------------------------------------------------------------------------------
    def _forward_impl(self, x, h0, c0, body, R, t, stash=True, x_src=None, pose_grad=False):
        """x_src, pose_grad: _UpperBase._front.  pose_grad: _backward_impl also forms d loss / d R and d loss / d t (pose_grads()); the
        head-frame transform's share needs the UNTRANSFORMED points: x_src when given (the caller leaves it alone until backward has
        run), else a copy taken here."""
        self.flat()
        ar = self.arena("train" if stash else "eval")
        feats, vec, attn, R, t = self._front(ar, x, x_src, R, t, stash, pose_grad)
        B, T, N, _ = x.shape
        body = _f32c(body)
        h0 = _f32c(h0) if h0 is not None else None
        c0 = _f32c(c0) if c0 is not None else None
        # sequence model, head and kinematics behind the per-frame feature vector (Net/Upper_Net.py:333-364,393-404)
        lstm = self.module1.grnn
        seq, hn, cn = blocks.lstm64_forward(ar, "grnn", lstm, vec, B, T, h0, c0, stash, self._drop_p(lstm) if stash else 0.0,
                                            self.seed_counter())
        l, q = self._head(ar, self.mlpHead.fc1, self.mlpHead.fc2, seq, body, B, T, R, t, stash)
        if stash:
            self._saved = (B, T, N, R, body, c0, attn)
        return l, q, attn, hn, cn

    def _front_fusable(self, Cx, N):
        layers = blocks._mlp3_layers(self.module0) + blocks._mlp3_layers(self.module1.gpointnet)
        dims = [tuple(conv.weight.shape[:2]) for conv, _ in layers]
        return (_FUSED_FRONT and Cx == 6 and N % 16 == 0 and 16 <= N <= 1024 and len({float(bn.eps) for _, bn in layers}) == 1
                and dims == [(8, 6), (16, 8), (24, 16), (32, 28), (48, 32), (64, 48)]
                and all(conv.bias is not None for conv, _ in layers) and self.module1.gpointnet.attn.bias is not None)

    def _front_table(self):
        """Host-side pointer table of mmego_upper_front_eval (38 device pointers)."""
        layers = blocks._mlp3_layers(self.module0) + blocks._mlp3_layers(self.module1.gpointnet)
        ts = [v for conv, bn in layers for v in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        return self._ptr_table("_front_tab", ts + [self.module1.gpointnet.attn.weight, self.module1.gpointnet.attn.bias])

    def _front_one_launch(self, x, x_src, R, t, vec, attn):
        """eval mode: transform, PointNet, concat, GlobalPointNet and the attention pooling as ONE launch (front.hip); the per-point
        28- / 64-channel tensors never exist in memory."""
        B, T, N, Cx = x.shape
        if self.training or not self._front_fusable(Cx, N):
            return False
        hip.call("upper_front_eval_bf16" if self._bf16_eval(False) else "upper_front_eval", x, x_src, R, t, B * T, N, self._front_table(),
                 float(self.module0.cb1.eps), vec, attn)
        return True

    def _backward_impl(self, dl, dl_extra=None, pose_add=None):
        """dl_extra (optional, [F,15,3]): a second gradient with respect to the predicted joints, added to dl's (the joint stage-3 step:
        Lower_Net's d upper_l beside this net's own loss gradient).  Behind a pose_grad forward the head pose's gradients cover both.
        pose_add (optional, (dR [F,3,3], dt [F,3]); needs dl_extra and a pose_grad forward): somebody else's gradients with respect to the
        same head pose (the three-net step: Lower_Net's), added to pose_grads()."""
        ar = self.arena("train")
        B, T, N, R, body, c0, attn = self._saved
        F = B * T
        G = self._flat.grad
        y, dy = ar.get("y", (F, 87)), ar.get("dy", (F, 87))
        pose = self._pose
        ready = getattr(self, "_dy_ready", False)
        if pose_add is not None and (dl_extra is None or pose is None):
            raise ValueError("UpperNet: pose_add goes with dl_extra behind a pose_grad forward")
        if dl_extra is not None:
            if ready:
                # the fused loss launch has left the own loss's dy (and its dR, dt): the kinematics' backward is linear in its input
                # gradient, so the second gradient's dy is added to it
                if pose is not None:
                    # ... and its world-transform share of dR, dt, and pose_add, by the same launch
                    hip.call("head_fk_backward_extra", 0, y, body, B, F, _f32c(dl_extra), dy, R, ar.get("jh", (F, 15, 3)), pose[2], pose[3],
                             *(pose_add if pose_add is not None else (None, None)))
                else:
                    dyx = ar.get("dy_extra", (F, 87))
                    self._head_fk_backward(ar, 0, y, body, B, F, _f32c(dl_extra), dyx, R, (F, 15, 3), None, second=True)
                    ops.copy2d(dyx, dy, accumulate=True)
            else:
                dls = ar.get("dl_sum", (F, 45))
                ops.copy2d(_f32c(dl).view(F, 45), dls)
                ops.copy2d(_f32c(dl_extra).view(F, 45), dls, accumulate=True)
                dl = dls
        dl = _f32c(dl) if dl is not None else None
        self._head_fk_backward(ar, 0, y, body, B, F, dl, dy, R, (F, 15, 3), pose[2:] if pose is not None else None)
        if pose_add is not None and not ready:
            ops.copy2d(_f32c(pose_add[0]).view(F, 9), pose[2].view(F, 9), accumulate=True)
            ops.copy2d(_f32c(pose_add[1]).view(F, 3), pose[3].view(F, 3), accumulate=True)
        leaves = []          # weight gradients of the head and of the BiLSTM stack: leaves, issued together behind the stack
        dseq = ar.get("dseq", (F, 128))
        self._head_backward(ar, self.mlpHead.fc1, self.mlpHead.fc2, ar.get("grnn.out2", (F, 128)), dseq, F, G, leaves)
        lstm = self.module1.grnn
        dvec = blocks.lstm64_backward(ar, "grnn", lstm, ar.get("vec", (F, 64)), B, T, c0, dseq, G, self._drop_p(lstm), True, leaves=leaves)
        blocks.run_leaves(leaves)
        with blocks.dw_reduce_group():                         # the two chains' weight-gradient partials: one reduce launch
            dfeats = self._global_backward(ar, F, N, attn, dvec, G)
            dpts = self._pointnet_backward(ar, F, N, dfeats, G)
        self._pose_head_share(F, N, R, dfeats, dpts)


# =====================================================================================================
# Lower_Net
# =====================================================================================================
class BasePointNet(_Mlp3):
    def __init__(self, hidden_dim=64):
        super().__init__((6, 16, 32, hidden_dim - 3))


class PointEncoder(nn.Module):
    def __init__(self, hidden_dim):
        super().__init__()
        self.module0 = BasePointNet(hidden_dim)


class _GraphConv(nn.Module):
    def __init__(self, cin, cout, K):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout * K, kernel_size=(1, 1))


class StGcnBlock(nn.Module):
    """Parameter container of one st_gcn block (reference Net/GCN.py:67-147)."""

    def __init__(self, cin, cout, K, taps=9):
        super().__init__()
        self.cin, self.cout, self.K, self.taps = cin, cout, K, taps
        self.gcn = _GraphConv(cin, cout, K)
        self.tcn = nn.ModuleDict({"0": nn.BatchNorm2d(cout),
                                  "2": nn.Conv2d(cout, cout, (taps, 1), (1, 1), (taps // 2, 0)),
                                  "3": nn.BatchNorm2d(cout)})
        self.residual = nn.ModuleDict({"0": nn.Conv2d(cin, cout, kernel_size=1, stride=(1, 1)),
                                       "1": nn.BatchNorm2d(cout)})


class Model(nn.Module):
    """ST-GCN container (reference Net/GCN.py:281-355); `extract_feature` runs inside LowerNet's pipeline."""

    def __init__(self, in_channels, hidden_dim, graph_args={}, edge_importance_weighting=True, **kwargs):
        super().__init__()
        A = torch.tensor(gcn_adjacency(graph_args.get("strategy", "uniform")), dtype=torch.float32)
        self.register_buffer("A", A)
        K = A.size(0)
        self.data_bn = nn.BatchNorm1d(in_channels * A.size(1))
        self.gcn_networks = nn.ModuleList((StGcnBlock(in_channels, 32, K), StGcnBlock(32, 64, K),
                                           StGcnBlock(64, 128, K)))
        if edge_importance_weighting:
            self.edge_importance = nn.ParameterList([nn.Parameter(torch.ones(A.size())) for _ in self.gcn_networks])
        else:
            raise NotImplementedError("edge_importance_weighting=False is not used by the reference nets")
        self.fcn = nn.Conv2d(128, hidden_dim, kernel_size=1)


class KeyEncoder(nn.Module):
    def __init__(self, hidden_dim):
        super().__init__()
        self.gcn = Model(in_channels=3, hidden_dim=hidden_dim, graph_args={"strategy": "distance"})


class FusionModule(nn.Module):
    def __init__(self, hidden_dim=64):
        super().__init__()
        self.fc0 = nn.Linear(hidden_dim * 2 + JOINTS_UPPER * 3, 128)
        self.fc1 = nn.Linear(128, 64)
        self.to_q = nn.Linear(hidden_dim, hidden_dim, bias=True)
        self.to_k = nn.Linear(hidden_dim, hidden_dim, bias=True)
        self.to_v = nn.Linear(hidden_dim, hidden_dim, bias=True)
        self.scale = hidden_dim ** -0.5
        self.fc2 = nn.Linear(64, 6 * 6 + 2 * 3)
        self.attn = nn.Linear(hidden_dim * 2, 1)       # Q6: its softmax runs over a size-1 axis -> no effect
        self.rnn_pk = LstmParams(hidden_dim * 3, hidden_dim, 3, dropout=0.1, bidirectional=True)


class LowerNet(_NetBase):
    """forward(upper_l[B,T,15,3], x[B,T,N,6], h0_p, c0_p, h0_k, c0_k, initial_body, R, t) -> (l[B,T,8,3], q[B,T,6,3,3]).
    The four state arguments are ignored, as in the reference (Q7).  MUTATES x (Q1).
    differentiable_inputs (default False: an upper_l, R or t that requires grad is refused): when True, such inputs receive their
    gradients from backward -- both head-frame transforms (selected points, predicted joints), everything the joints feed (ST-GCN,
    fc0) and, for R and t, the world transform behind the kinematics.  x and initial_body are not differentiable."""

    differentiable_inputs = False

    def __init__(self, hidden_dim):
        super().__init__()
        if hidden_dim != 64:
            raise ValueError("LowerNet: hidden_dim must be 64 (the reference hard-codes BatchNorm1d(61))")
        self.pointEncoder = PointEncoder(hidden_dim)
        self.keyEncoder = KeyEncoder(hidden_dim)
        self.fusion = FusionModule(hidden_dim)

    def _pulled_pairs(self):
        """Besides the BiLSTM pairs: per st_gcn block the graph convolution's and the residual branch's k=1 conv weights (both
        read the block input: one stacked [3 cout, cin] product forward, one weight-gradient and one input-gradient product
        backward) and their biases; the fusion attention's key and value projections likewise."""
        pulled = super()._pulled_pairs()
        for i in range(len(self.keyEncoder.gcn.gcn_networks)):
            pre = "keyEncoder.gcn.gcn_networks.%d." % i
            pulled[pre + "gcn.conv.weight"] = pre + "residual.0.weight"
            pulled[pre + "gcn.conv.bias"] = pre + "residual.0.bias"
        pulled["fusion.to_k.weight"] = "fusion.to_v.weight"          # key / value projections of the same skeleton features
        pulled["fusion.to_k.bias"] = "fusion.to_v.bias"
        return pulled

    def forward(self, upper_l, x, h0_p, c0_p, h0_k, c0_k, initial_body, R, t, pin_select_idx=None):
        """``pin_select_idx`` [B*T, 64] int64 (tests only; not in the reference's signature): use these point indices instead of
        the kernel's own top-64-by-x selection.  torch.sort in the reference is unstable, so where equal x keys straddle the
        cut its choice depends on the torch build; replaying the recorded choice lets the HIP path be compared with the
        reference's outputs (goldens G5 / G9) at the 1e-3 cm bar instead of through the oracle alone."""
        _require_gpu(x, "LowerNet")
        if not self.differentiable_inputs:
            _refuse_pose_grad("LowerNet", upper_l=upper_l, R=R, t=t)
        elif _pose_wants_grad(upper_l, R, t):
            self.flat()
            return _InputBridge.apply(self, (x, initial_body, pin_select_idx), upper_l, R, t, *self._flat.params)
        return self._bridged((upper_l, x, initial_body, R, t, pin_select_idx))

    def input_grads(self):
        """(d upper_l [F,15,3] | None, dR [F,3,3] | None, dt [F,3] | None) of the last backward behind an input_grad forward: arena
        buffers, rewritten by the next one."""
        ig = getattr(self, "_ingrad", None)
        if ig is None:
            raise RuntimeError("LowerNet.input_grads: the last forward did not ask for input gradients")
        return ig["d_upper_l"], ig["dR"], ig["dt"]

    def _forward_impl(self, upper_l, x, body, R, t, pin_select_idx=None, stash=True, input_grad=()):
        """input_grad: a subset of {"upper_l", "pose"} -- _backward_impl also forms d loss / d upper_l, respectively d loss / d R and
        d loss / d t (input_grads()).  "pose" keeps a copy of the points as they arrive (the second transform's UNTRANSFORMED input: x is
        transformed in place), asks BasePointNet for its input gradient and takes the world transform's share from the kinematics
        launch; "upper_l" alone costs none of these."""
        self.flat()
        training = self.training
        ar = self.arena("train" if stash else "eval")
        if not (x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("LowerNet: x must be a contiguous fp32 tensor (it is transformed in place)")
        B, T, N, Cx = x.shape
        F = B * T
        V = JOINTS_UPPER
        dev = x.device
        R, t, body = _f32c(R), _f32c(t), _f32c(body)
        up = ar.get("up", (F, V * 3))
        upper_l = _f32c(upper_l)
        self._ingrad = None
        want = frozenset(input_grad)
        if want:
            if not stash or not want <= {"upper_l", "pose"}:
                raise ValueError("LowerNet: input_grad is a subset of {'upper_l', 'pose'} and needs a forward that keeps its "
                                 "activations (stash=True)")
            pose = "pose" in want
            raw = None
            if pose:
                raw = ar.get("pts_raw", (F * N, Cx))
                ops.copy2d(x.view(F * N, Cx), raw)
            self._ingrad = dict(upper_l=upper_l, raw=raw, t=t, d_upper_l=ar.get("d_upper_l", (F, V, 3)) if "upper_l" in want else None,
                                dR=ar.get("dR", (F, 3, 3)) if pose else None, dt=ar.get("dt", (F, 3)) if pose else None)
        # Q1 (second transform after UpperNet) and the predicted joints' copy + transform: one launch
        hip.call("transform2h_pair", x, F, N, Cx, R, t, up, V, upper_l)
        sel = ar.get("sel", (F * LOWER_POINTS, Cx))
        idx = ar.get("sel_idx", (F, LOWER_POINTS), dtype=torch.int64)
        prow = F * LOWER_POINTS
        # training: [p_vec | cross-attention output] in one buffer (p_vec is written in place; backward reads both halves).  Eval (r06):
        # p_vec alone, contiguous -- the attention output is pooled over the points inside its own launch and never stored
        both = ar.get("both", (prow, 128)) if training else None
        p_vec = both[:, :64] if training else ar.get("p_vec", (prow, 64))
        # the xyz part of p_vec: in training from the selection launch itself (one launch less in a latency-bound chain); in eval mode
        # from BasePointNet's launch, next to the features of the same rows (r06: at config 5 the selection's 12 bytes into every
        # 512-byte row of a 1-GB buffer cost 150 us of isolated partial-line writes)
        front = None if training else p_vec[:, :3]
        if pin_select_idx is None:
            if training:
                hip.call("topk_rows2", x, F, N, Cx, LOWER_POINTS, sel, idx, p_vec, both.stride(0), 3)
            else:
                hip.call("topk_rows", x, F, N, Cx, LOWER_POINTS, sel, idx)
        else:                                                         # replay a recorded selection (see forward)
            pin = pin_select_idx.to(device=dev, dtype=torch.int64).reshape(F, LOWER_POINTS)
            if int(pin.min()) < 0 or int(pin.max()) >= N:
                raise ValueError("pin_select_idx out of range")
            idx.copy_(pin)
            flat_idx = (pin + torch.arange(F, device=dev, dtype=torch.int64).view(F, 1) * N).reshape(-1).contiguous()
            ops.gather_rows(x.view(F * N, Cx), flat_idx, sel)
            if training:
                ops.copy2d(sel[:, :3], p_vec[:, :3])
        self.last_select_idx = idx
        blocks.mlp3_forward(ar, "base", self.pointEncoder.module0, sel, p_vec[:, 3:64], training, bf16=self._bf16_eval(training), front=front)

        k_vec = self._gcn_forward(ar, up, B, T, training)            # [F*15, 64] in the re-viewed layout (Q8)

        fu = self.fusion
        KVm = ar.get("KVm", (F * V, 128))
        Km, Vm = KVm[:, :64], KVm[:, 64:]
        Wq = fu.to_q.weight.view(64, -1)
        fuse_q = (not training) and Wq.shape == (64, 64) and Wq.is_contiguous() and fu.to_q.bias is not None      # (eval: inside the attention launch)
        if not fuse_q:
            Qm = ar.get("Qm", (prow, 64))
            ops.linear(p_vec, fu.to_q.weight, fu.to_q.bias, Qm)
        Wkv, bkv = ops.stacked(fu.to_k.weight, fu.to_v.weight), ops.stacked(fu.to_k.bias, fu.to_v.bias)
        if Wkv is not None and bkv is not None:                 # keys and values: one stacked product (flat_param_order)
            ops.linear(k_vec, Wkv, bkv, KVm)
        else:
            ops.linear(k_vec, fu.to_k.weight, fu.to_k.bias, Km)
            ops.linear(k_vec, fu.to_v.weight, fu.to_v.bias, Vm)
        ak = ar.get("ak", (F, 192))
        if training:
            Pm = ar.get("Pm", (F, LOWER_POINTS, V))
            hip.call("cross_attn_forward", Qm, Km, Vm, F, float(fu.scale), both[:, 64:], 128, Pm, 128)
            # Q6: gate == 1 -> plain sum over the points; mean over the joints: one launch for both
            hip.call("group_sum2", F, both, LOWER_POINTS, 128, 1.0, ak, 192, k_vec, V, 64, 1.0 / V, ak[:, 128:], 192)
        else:
            # the attention output summed over the points by the attention launch (same order of addition as group_sum2: same bits),
            # straight into its columns of ak; the p_vec half and the joints' mean as before
            if fuse_q:                  # ... and the queries computed there too: Q is never stored
                hip.call("cross_attn_forward_pooled_q", p_vec, p_vec.stride(0), Wq, fu.to_q.bias, Km, Vm, F, float(fu.scale), ak[:, 64:], 192, 128)
            else:
                hip.call("cross_attn_forward_pooled", Qm, Km, Vm, F, float(fu.scale), ak[:, 64:], 192, 128)
            hip.call("group_sum2", F, p_vec, LOWER_POINTS, 64, 1.0, ak, 192, k_vec, V, 64, 1.0 / V, ak[:, 128:], 192)
        lstm = fu.rnn_pk
        seq, _, _ = blocks.lstm64_forward(ar, "rnn", lstm, ak, B, T, None, None, stash, self._drop_p(lstm) if stash else 0.0,
                                          self.seed_counter())
        cat = ar.get("cat", (F, 173))
        hip.call("copy2d_pair", seq, seq.stride(0), cat, cat.stride(0), F, 128, up, up.stride(0), cat[:, 128:173], cat.stride(0), F, 45)
        f0, f1, y = ar.get("f0", (F, 128)), ar.get("f1", (F, 64)), ar.get("y", (F, 42))
        ops.linear(cat, fu.fc0.weight, fu.fc0.bias, f0, relu=True)
        ops.linear(f0, fu.fc1.weight, fu.fc1.bias, f1, relu=True)
        ops.linear(f1, fu.fc2.weight, fu.fc2.bias, y)
        q = torch.empty((B, T, 6, 3, 3), dtype=torch.float32, device=dev)
        jh = ar.get("jh", (F, 8, 3))
        l = torch.empty((B, T, 8, 3), dtype=torch.float32, device=dev)
        tick = self._flat.tick_args(self.seed_counter()) if training else (None, 0, None)   # BatchNorm counters + dropout seed
        ig = self._ingrad
        # kinematics + head-to-world transform (+ loss), one launch
        self._head_fk(ar, 1, y, body, B, F, q, jh, R, t, l, tick, stash, pose=(ig["dR"], ig["dt"]) if (ig is not None and ig["dR"] is not None) else None)
        if stash:
            self._saved = (B, T, N, R, body)
        return l, q

    def _packed_tconv(self, i, wt, taps):
        """Temporal-conv weight of block i re-packed [tap][co][ci] (k-contiguous tile loads) for eval-mode forwards; rebuilt
        only when the weight tensor changed."""
        cache = self.__dict__.setdefault("_tconv_packed", {})
        ver = (wt._version, wt.data_ptr())
        ent = cache.get(i)
        if ent is None or ent[0] != ver:
            wp = torch.empty(wt.numel(), dtype=torch.float32, device=wt.device)
            hip.call("tconv_pack", wt, wt.shape[0], wt.shape[1], taps, 0, wp)
            ent = cache[i] = (ver, wp)
        return ent[1]

    # -- ST-GCN (Net/GCN.py:332-355) on channels-last rows (b,t,v) ------------------------------------
    def _gcn_fusable(self, B, T):
        """The fused training kernels' shape limits (gcn_fused.hip): <= 1024 frames (data_bn's statistics are taken by every
        workgroup; <= 256 partial records per BatchNorm), the reference's channel ladder, K <= 3 partitions."""
        gcn = self.keyEncoder.gcn
        blks = gcn.gcn_networks
        ok = _GCN_FUSED and B * T <= 1024 and len(blks) == 3 and gcn.A.shape[1] == JOINTS_UPPER and gcn.A.shape[0] <= 3
        ok = ok and blks[0].cin * JOINTS_UPPER <= 64 and [b.cout for b in blks] == [32, 64, 128] and all(b.taps == 9 for b in blks)
        ok = ok and gcn.fcn.weight.shape[0] == 64 and gcn.A.is_contiguous()
        for blk in blks:
            ok = ok and ops.stacked(blk.gcn.conv.weight.view(blk.K * blk.cout, blk.cin), blk.residual["0"].weight.view(blk.cout, blk.cin)) is not None
            ok = ok and ops.stacked(blk.gcn.conv.bias, blk.residual["0"].bias) is not None
        return bool(ok)

    def _gcn_forward_fused(self, ar, up, B, T):
        """Training forward of the ST-GCN in 8 launches (one weight pack, per block gcn_front + tconv_train, the closing conv):
        BatchNorm statistics travel as partial records and are finalized in the consumers' prologues (gcn_fused.hip)."""
        gcn = self.keyEncoder.gcn
        V = JOINTS_UPPER
        F, rows = B * T, B * T * V
        nrf, nrt = hip.lib().mmego_gcn_front_nrec(F), (rows + 63) // 64
        blks = gcn.gcn_networks
        wps = [ar.get("gcn.b%d.wp" % i, (2, blk.tcn["2"].weight.numel())) for i, blk in enumerate(blks)]
        # every weight re-layout of the step in one launch: the temporal convs' tap-major packs (forward + gradient) and the
        # fragment-major copies of the stacked 1x1 weights gcn_front multiplies with (blocks with cin >= 32, and fcn)
        seq = [blk.taps == 9 and bool(hip.lib().mmego_tconv_seq_ok(T, V, blk.cout, blk.cout)) for blk in blks]      # sequence-tiled temporal conv (gcn.hip)
        self._tconv_seq = seq
        packs = [hip.Pack(hip.ptr(blk.tcn["2"].weight), hip.ptr(wp), blk.cout, blk.cout, blk.taps, 2 if sq else 0)
                 for blk, wp, sq in zip(blks, wps, seq)]
        wfr = {}
        for i, blk in enumerate(blks):
            if blk.cin >= 32:
                Wc = ops.stacked(blk.gcn.conv.weight.view(blk.K * blk.cout, blk.cin), blk.residual["0"].weight.view(blk.cout, blk.cin))
                wfr[i] = ar.get("gcn.b%d.wfrag" % i, (Wc.numel(),))
                packs.append(hip.Pack(hip.ptr(Wc), hip.ptr(wfr[i]), Wc.shape[0], blk.cin, 1, 1))
        wfr["fcn"] = ar.get("gcn.fcn.wfrag", (gcn.fcn.weight.numel(),))
        packs.append(hip.Pack(hip.ptr(gcn.fcn.weight), hip.ptr(wfr["fcn"]), 64, gcn.fcn.weight.shape[1], 1, 1))
        hip.call("pack_multi", len(packs), (hip.Pack * len(packs))(*packs))
        prev = None
        for i, blk in enumerate(blks):
            cin, cout, K = blk.cin, blk.cout, blk.K
            key = "gcn.b%d" % i
            zr = ar.get(key + ".zr", (rows, (K + 1) * cout))
            ymix, tz, y0 = ar.get(key + ".ymix", (rows, cout)), ar.get(key + ".tz", (rows, cout)), ar.get(key + ".y0", (rows, cout))
            n3, r3 = (B, T * V) if seq[i] else (nrt, 64)                  # records of the temporal conv's output: per sequence / per 64-row tile
            recY, recR, rec3 = ar.get(key + ".recY", (nrf, cout, 2)), ar.get(key + ".recR", (nrf, cout, 2)), ar.get(key + ".rec3", (n3, cout, 2))
            d = hip.GcnFront()
            if prev is None:
                d.X1, d.ld1, d.in_mode = hip.ptr(up), V * cin, 0
                d.bn1 = hip.BnRef.of(gcn.data_bn, ops.BnState(ar, "gcn.dbn", V * cin).all)
                d.xact = hip.ptr(ar.get("gcn.x0", (F, V * cin)))
            else:
                ptz, pzr, prec3, precR, pblk, pkey, pn3, pr3 = prev
                pc = pblk.cout
                d.X1, d.ld1, d.X2, d.ld2, d.in_mode = hip.ptr(ptz), pc, hip.ptr(pzr[:, pblk.K * pc:]), pzr.stride(0), 1
                d.bn1 = hip.BnRef.of(pblk.tcn["3"], ops.BnState(ar, pkey + ".bn3", pc).all, prec3, pn3, pr3)
                d.bn2 = hip.BnRef.of(pblk.residual["1"], ops.BnState(ar, pkey + ".bnr", pc).all, precR, nrf, 4 * V)
                d.xact = hip.ptr(ar.get(pkey + ".out", (rows, pc)))
            Wc = ops.stacked(blk.gcn.conv.weight.view(K * cout, cin), blk.residual["0"].weight.view(cout, cin))
            bc = ops.stacked(blk.gcn.conv.bias, blk.residual["0"].bias)
            d.W, d.bias, d.cin, d.nout = hip.ptr(wfr.get(i, Wc)), hip.ptr(bc), cin, (K + 1) * cout
            d.mix, d.K, d.cout, d.A, d.importance = 1, K, cout, hip.ptr(gcn.A), hip.ptr(gcn.edge_importance[i])
            d.Z, d.ldz, d.Y, d.recY, d.recR = hip.ptr(zr), zr.stride(0), hip.ptr(ymix), hip.ptr(recY), hip.ptr(recR)
            d.F, d.V = F, V
            hip.call("gcn_front", d)
            bn0 = hip.BnRef.of(blk.tcn["0"], ops.BnState(ar, key + ".bn0", cout).all, recY, nrf, 4 * V)
            hip.call("tconv_seq_train" if seq[i] else "tconv_train", ymix, cout, bn0, wps[i][0], blk.tcn["2"].bias, tz, cout, y0, rec3,
                     B, T, V, cout, cout, blk.taps)
            prev = (tz, zr, rec3, recR, blk, key, n3, r3)
        ptz, pzr, prec3, precR, pblk, pkey, pn3, pr3 = prev
        pc = pblk.cout
        kv = ar.get("gcn.kv", (B, 64, T * V))
        d = hip.GcnFront()
        d.X1, d.ld1, d.X2, d.ld2, d.in_mode = hip.ptr(ptz), pc, hip.ptr(pzr[:, pblk.K * pc:]), pzr.stride(0), 1
        d.bn1 = hip.BnRef.of(pblk.tcn["3"], ops.BnState(ar, pkey + ".bn3", pc).all, prec3, pn3, pr3)
        d.bn2 = hip.BnRef.of(pblk.residual["1"], ops.BnState(ar, pkey + ".bnr", pc).all, precR, nrf, 4 * V)
        d.xact = hip.ptr(ar.get(pkey + ".out", (rows, pc)))
        d.W, d.bias, d.cin, d.nout = hip.ptr(wfr["fcn"]), hip.ptr(gcn.fcn.bias), pc, 64
        d.mix, d.outT, d.T, d.F, d.V = 0, hip.ptr(kv), T, F, V
        hip.call("gcn_front", d)
        return kv.view(F * V, 64)

    # -- eval-mode ST-GCN with bf16 operands (gcn_bf16.hip) ------------------------------------------
    def _gcn_bf16_ok(self, B, T):
        gcn = self.keyEncoder.gcn
        V, lib = JOINTS_UPPER, hip.lib()
        ok = gcn.A.is_contiguous() and gcn.A.shape[1] == V
        for blk in gcn.gcn_networks:
            ok = ok and bool(lib.mmego_gcn_mix_eval_bf16_ok(V, blk.cin, blk.cout, blk.K))
            ok = ok and bool(lib.mmego_tconv_eval_bf16_ok(T, V, blk.cout, blk.cout, blk.taps))
        return bool(ok)

    def _gcn_pack_bf16(self):
        """Everything the bf16 eval blocks read besides activations, built once per weight version: the 1x1 weights as bf16
        fragment-major matrices over the k axis [A_0^T X | A_1^T X | A_2^T X | X] (include/mmego_hip.h), the einsum's bias table,
        the temporal weights in their chunk order, the frozen BatchNorms as [4][C] states (mean, invstd, a, b)."""
        gcn = self.keyEncoder.gcn
        src = list(gcn.parameters()) + list(gcn.buffers())
        ver = tuple((t._version, t.data_ptr()) for t in src)
        ent = self.__dict__.get("_gcn_bf16_pack")
        if ent is not None and ent[0] == ver:
            return ent[1]
        dev = gcn.A.device

        def state(bn):
            C = bn.weight.numel()
            st = torch.empty((4, C), dtype=torch.float32, device=dev)
            hip.call("bn_eval_affine", C, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps), st[0], st[1], st[2], st[3])
            return st

        def frag(Wm):                                          # [cout][16 ns] fp32 -> bf16 [cout / 32][ns][lane half][32][8]
            co, kd = Wm.shape
            return Wm.to(torch.bfloat16).view(co // 32, 32, kd // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()

        with torch.no_grad():
            pk = {"dbn": state(gcn.data_bn), "blocks": []}
            for i, blk in enumerate(gcn.gcn_networks):
                cin, cout, K = blk.cin, blk.cout, blk.K
                kd = ((K + 1) * cin + 15) // 16 * 16
                ksy, kr0 = (K * cin + 15) // 16, (K * cin) // 16
                Wcat = torch.zeros((cout, kd), dtype=torch.float32, device=dev)
                Wcat[:, :K * cin] = blk.gcn.conv.weight.view(K, cout, cin).permute(1, 0, 2).reshape(cout, K * cin)
                Wy = Wcat[:, :ksy * 16].clone()
                Wcat.zero_()
                Wcat[:, K * cin:(K + 1) * cin] = blk.residual["0"].weight.view(cout, cin)
                Wr = Wcat[:, kr0 * 16:].clone()
                AI = gcn.A * gcn.edge_importance[i]
                biasy = torch.einsum("kw,kc->wc", AI.sum(dim=1), blk.gcn.conv.bias.view(K, cout)).contiguous()
                wt = blk.tcn["2"].weight
                Wt = torch.empty(wt.numel(), dtype=torch.bfloat16, device=dev)
                hip.call("tconv_pack_bf16", wt.contiguous(), cout, cout, blk.taps, Wt)
                pk["blocks"].append({"Wy": frag(Wy), "Wr": frag(Wr), "biasy": biasy, "biasr": blk.residual["0"].bias.detach().clone(),
                                     "st0": state(blk.tcn["0"]), "st3": state(blk.tcn["3"]), "st_r": state(blk.residual["1"]),
                                     "Wt": Wt, "bt": blk.tcn["2"].bias.detach().clone()})
        self.__dict__["_gcn_bf16_pack"] = (ver, pk)
        return pk

    def _gcn_forward_bf16(self, ar, up, B, T):
        """Eval forward of the three ST-GCN blocks in six launches, dense products on bf16 operands (gcn_bf16.hip)."""
        gcn = self.keyEncoder.gcn
        V = JOINTS_UPPER
        F, rows = B * T, B * T * V
        pk = self._gcn_pack_bf16()
        cur, in_state = _f32c(up).view(F, -1), pk["dbn"]
        for i, blk in enumerate(gcn.gcn_networks):
            cin, cout, K = blk.cin, blk.cout, blk.K
            key, bk = "gcn.b%d" % i, pk["blocks"][i]
            yact = ar.get(key + ".yact16", (rows, cout), dtype=torch.bfloat16)
            rn, out = ar.get(key + ".rn", (rows, cout)), ar.get(key + ".out", (rows, cout))
            hip.call("gcn_mix_eval_bf16", cur, in_state, gcn.A, gcn.edge_importance[i], bk["Wy"], bk["Wr"], bk["biasy"], bk["biasr"],
                     bk["st0"], bk["st_r"], yact, rn, F, V, cin, cout, K)
            hip.call("tconv_eval_bf16", yact, bk["Wt"], bk["bt"], bk["st3"], rn, cout, out, cout, 1, B, T, V, cout, cout, blk.taps)
            cur, in_state = out, None
        return cur

    def _gcn_forward(self, ar, up, B, T, training):
        gcn = self.keyEncoder.gcn
        V = JOINTS_UPPER
        F, rows = B * T, B * T * V
        self._gcn_was_fused = bool(training and self._gcn_fusable(B, T))
        if self._gcn_was_fused:
            return self._gcn_forward_fused(ar, up, B, T)
        if self._bf16_eval(training) and self._gcn_bf16_ok(B, T):
            cur = self._gcn_forward_bf16(ar, up, B, T)
            return self._gcn_fcn(ar, cur, B, T)
        st = ops.bn_stats(ar, "gcn.dbn", up, gcn.data_bn, training)
        x0 = ar.get("gcn.x0", (F, V * 3))
        ops.affine_act(up, st, x0, relu=False)
        cur = x0.view(rows, 3)
        for i, blk in enumerate(gcn.gcn_networks):
            cin, cout, K = blk.cin, blk.cout, blk.K
            key = "gcn.b%d" % i
            # the graph convolution's and the residual branch's k=1 convs read the same input: one product with the stacked
            # weight [K cout + cout, cin] (the two tensors are neighbours in the flat buffer: flat_param_order), outputs side by
            # side in one buffer
            zr = ar.get(key + ".zr", (rows, (K + 1) * cout))
            z, res_z = zr[:, :K * cout], zr[:, K * cout:]
            Wc = ops.stacked(blk.gcn.conv.weight.view(K * cout, cin), blk.residual["0"].weight.view(cout, cin))
            bc = ops.stacked(blk.gcn.conv.bias, blk.residual["0"].bias)
            if Wc is not None and bc is not None:
                ops.linear(cur, Wc, bc, zr)
            else:
                ops.linear(cur, blk.residual["0"].weight, blk.residual["0"].bias, res_z)
                ops.linear(cur, blk.gcn.conv.weight, blk.gcn.conv.bias, z)
            ymix = ar.get(key + ".ymix", (rows, cout))
            # einsum('nkctv,kvw->nctw', z, A * edge_importance): one launch, A . importance formed in LDS (gcn.hip)
            if training and F <= 1024:
                # the einsum leaves the BatchNorm partials of its output (one record per frame and channel) beside it
                ws = ops.scratch(z.device, 3 * cout * F)
                hip.call("graph_mix", z, gcn.A, gcn.edge_importance[i], ymix, F, V, K, cout, 0, ws, z.stride(0))
                st0 = ops.BnState(ar, key + ".bn0", cout)
                bn0 = blk.tcn["0"]
                hip.call("bn_finalize", ws, F, cout, bn0.weight, bn0.bias, bn0.running_mean, bn0.running_var, float(bn0.momentum),
                         float(bn0.eps), st0.mean, st0.invstd, st0.a, st0.b)
            else:
                hip.call("graph_mix", z, gcn.A, gcn.edge_importance[i], ymix, F, V, K, cout, 0, None, z.stride(0))
                st0 = ops.bn_stats(ar, key + ".bn0", ymix, blk.tcn["0"], training)
            tz = ar.get(key + ".tz", (rows, cout))
            wt = blk.tcn["2"].weight                          # [cout, cout, taps, 1]
            # 9x1 temporal convolution, implicit (gcn.hip): BatchNorm + ReLU applied while the tiles are loaded; a training step
            # keeps the activated rows y0 (they leave from the same launch) and packs the weights for both of its uses
            if training:
                y0 = ar.get(key + ".y0", (rows, cout))
                wp = ar.get(key + ".wp", (2, wt.numel()))
                hip.call("tconv_pack", wt, cout, cout, blk.taps, 2, wp)
                hip.call("tconv", ymix, cout, st0.all, wp[0], blk.tcn["2"].bias, tz, cout, y0, B, T, V, cout, cout, blk.taps)
            else:
                hip.call("tconv", ymix, cout, st0.all, self._packed_tconv(i, wt, blk.taps), blk.tcn["2"].bias, tz, cout, None,
                         B, T, V, cout, cout, blk.taps)
            # the block's two closing BatchNorms (temporal branch, residual branch) in one pair of launches
            st3, st_r = ops.bn_stats_pair(ar, key + ".bn3", tz, blk.tcn["3"], key + ".bnr", res_z, blk.residual["1"], training)
            out = ar.get(key + ".out", (rows, cout))
            ops.affine_act(tz, st3, out, relu=True, X2=res_z, st2=st_r)
            cur = out
        return self._gcn_fcn(ar, cur, B, T)

    def _gcn_fcn(self, ar, cur, B, T):
        gcn = self.keyEncoder.gcn
        V = JOINTS_UPPER
        F, rows = B * T, B * T * V
        kv = ar.get("gcn.kv", (B, 64, T * V))
        if rows <= 16384:
            # fcn as one product per sequence b with a TRANSPOSED store: (B,T*V,128) -> (B,64,T*V), then re-viewed (Q8); no
            # transpose launch (small shapes: the strided store is not coalesced)
            ops.bmm(cur.view(B, T * V, cur.shape[1]), gcn.fcn.weight.view(64, -1).t().unsqueeze(0).expand(B, -1, -1),
                    kv.transpose(1, 2), bias=gcn.fcn.bias)
        else:
            fz = ar.get("gcn.fz", (rows, 64))
            ops.linear(cur, gcn.fcn.weight, gcn.fcn.bias, fz)
            hip.call("transpose_batched", fz, kv, B, T * V, 64)       # (B,T*V,64) -> (B,64,T*V), then re-viewed (Q8)
        return kv.view(F * V, 64)

    def _backward_impl(self, dl):
        ar = self.arena("train")
        B, T, N, R, body = self._saved
        F, V = B * T, JOINTS_UPPER
        prow = F * LOWER_POINTS
        G = self._flat.grad
        fu = self.fusion
        dl = _f32c(dl)
        y, f1, f0, cat = ar.get("y", (F, 42)), ar.get("f1", (F, 64)), ar.get("f0", (F, 128)), ar.get("cat", (F, 173))
        dy = ar.get("dy", (F, 42))
        ig = getattr(self, "_ingrad", None)
        pose = ig is not None and ig["dR"] is not None
        self._head_fk_backward(ar, 1, y, body, B, F, dl, dy, R, (F, 8, 3), (ig["dR"], ig["dt"]) if pose else None)
        df1, df0, dcat = ar.get("df1", (F, 64)), ar.get("df0", (F, 128)), ar.get("dcat", (F, 173))
        leaves = []          # weight gradients of the fusion head and of the BiLSTM stack: leaves, issued together behind the stack
        blocks.linear_backward(dy, f1, fu.fc2, G, df1, relu_input=True, leaves=leaves)
        blocks.linear_backward(df1, f0, fu.fc1, G, df0, relu_input=True, leaves=leaves)
        blocks.linear_backward(df0, cat, fu.fc0, G, dcat, leaves=leaves)
        lstm = fu.rnn_pk
        ak = ar.get("ak", (F, 192))
        dak = blocks.lstm64_backward(ar, "rnn", lstm, ak, B, T, None, dcat[:, :128], G, self._drop_p(lstm), True, leaves=leaves)
        blocks.run_leaves(leaves)
        dboth = ar.get("dboth", (prow, 128))
        dk = ar.get("dk", (F * V, 64))
        hip.call("group_bcast2", F, dak, 192, LOWER_POINTS, 128, 1.0, dboth, dak[:, 128:], 192, V, 64, 1.0 / V, dk)
        dp = dboth[:, :64]           # (accumulated into in place: the attention's input gradient reads the other half)
        Qm, KVm = ar.get("Qm", (prow, 64)), ar.get("KVm", (F * V, 128))
        Km, Vm = KVm[:, :64], KVm[:, 64:]
        Pm = ar.get("Pm", (F, LOWER_POINTS, V))
        dQ, dKV = ar.get("dQ", (prow, 64)), ar.get("dKV", (F * V, 128))
        dK, dV = dKV[:, :64], dKV[:, 64:]
        hip.call("cross_attn_backward", Qm, Km, Vm, Pm, dboth[:, 64:], 128, F, float(fu.scale), dQ, dK, dV, 128)
        p_vec = ar.get("both", (prow, 128))[:, :64]
        k_vec = ar.get("gcn.kv", (B, 64, T * V)).view(F * V, 64)
        # split-K / split-row partial products of this backward pass are summed by ONE launch at its end (ops.SlabList)
        slabs = ops.SlabList() if getattr(self, "_gcn_was_fused", False) else None
        Wkv = ops.stacked(fu.to_k.weight, fu.to_v.weight)
        gWkv, gbkv = ops.stacked(G(fu.to_k.weight), G(fu.to_v.weight)), ops.stacked(G(fu.to_k.bias), G(fu.to_v.bias))
        if slabs is not None:
            ops.grad_weight_deferred(dQ, p_vec, G(fu.to_q.weight), slabs, ar, "slab.to_q", db=G(fu.to_q.bias))
            ops.grad_input(dQ, fu.to_q.weight, dp, accumulate=True)
        else:
            blocks.linear_backward(dQ, p_vec, fu.to_q, G, dp, accumulate_dx=True)
        if Wkv is not None and gWkv is not None and gbkv is not None:
            if slabs is not None:
                ops.grad_weight_deferred(dKV, k_vec, gWkv, slabs, ar, "slab.to_kv", db=gbkv)
            else:
                ops.grad_weight(dKV, k_vec, gWkv, db=gbkv)          # both projections' gradients from the stacked products
            ops.grad_input(dKV, Wkv, dk, accumulate=True)
        else:
            blocks.linear_backward(dK, k_vec, fu.to_k, G, dk, accumulate_dx=True)
            blocks.linear_backward(dV, k_vec, fu.to_v, G, dk, accumulate_dx=True)
        sel = ar.get("sel", (prow, 6))
        dsel = blocks.mlp3_backward(ar, "base", self.pointEncoder.module0, sel, p_vec[:, 3:64], dp[:, 3:64], G, pose)
        if slabs is not None:
            self._gcn_backward_fused(ar, dk, B, T, G, slabs, input_grad=ig is not None)
            slabs.run()
        else:
            self._gcn_backward(ar, dk, B, T, G)
        if ig is not None:
            # the head-frame transforms' shares.  The transformed joints feed fc0 (dcat's last 45 columns) and data_bn (gcn.dup); the
            # selected points' transformed xyz feed BasePointNet's first layer (dsel) and the first columns of p_vec (dp)
            dup = ar.get("gcn.dup", (F, V * 3))
            dj = dcat[:, 128:173]
            idx = ar.get("sel_idx", (F, LOWER_POINTS), dtype=torch.int64)
            if pose:
                hip.call("lower_inputs_backward", ig["raw"], ig["raw"].stride(0), F, N, idx, LOWER_POINTS, R, ig["t"], dsel, dsel.stride(0),
                         dp, dp.stride(0), ig["upper_l"], V, dj, dj.stride(0), dup, dup.stride(0), 1, ig["dR"], ig["dt"], ig["d_upper_l"])
            else:
                hip.call("lower_inputs_backward", None, 0, F, N, None, LOWER_POINTS, R, ig["t"], None, 0, None, 0,
                         ig["upper_l"], V, dj, dj.stride(0), dup, dup.stride(0), 0, None, None, ig["d_upper_l"])

    def _gcn_backward_fused(self, ar, dk, B, T, G, slabs, input_grad=False):
        """Backward of the fused ST-GCN step: per block reduce + apply of the closing BatchNorm pair, the temporal convolution's weight
        and input gradient (the latter with the next BatchNorm's sums in its epilogue), both einsum gradients with that BatchNorm's
        backward applied on load, the stacked 1x1 convs' weight gradient (slabs deferred) and input gradient: 7 launches (was 14)."""
        gcn = self.keyEncoder.gcn
        V = JOINTS_UPPER
        F, rows = B * T, B * T * V
        nrt = (rows + 63) // 64
        dfz = ar.get("gcn.dfz", (rows, 64))
        hip.call("transpose_batched", dk, dfz, B, 64, T * V)      # (B,64,T*V) -> (B,T*V,64)
        cur = ar.get("gcn.b2.out", (rows, 128))
        dcur = ar.get("gcn.d3", (rows, 128))
        ops.grad_weight_deferred(dfz, cur, G(gcn.fcn.weight), slabs, ar, "slab.fcn", db=G(gcn.fcn.bias))
        ops.grad_input(dfz, gcn.fcn.weight, dcur)
        for i in (2, 1, 0):
            blk = gcn.gcn_networks[i]
            cin, cout, K = blk.cin, blk.cout, blk.K
            key = "gcn.b%d" % i
            inp = ar.get("gcn.b%d.out" % (i - 1), (rows, cin)) if i > 0 else ar.get("gcn.x0", (F, V * 3)).view(rows, 3)
            out, tz = ar.get(key + ".out", (rows, cout)), ar.get(key + ".tz", (rows, cout))
            zr = ar.get(key + ".zr", (rows, (K + 1) * cout))
            z, res_z = zr[:, :K * cout], zr[:, K * cout:]
            st3, st_r, st0 = ops.BnState(ar, key + ".bn3", cout), ops.BnState(ar, key + ".bnr", cout), ops.BnState(ar, key + ".bn0", cout)
            dtz = ar.get(key + ".dtz", (rows, cout))
            dzr = ar.get(key + ".dzr", (rows, (K + 1) * cout))
            dz, drz = dzr[:, :K * cout], dzr[:, K * cout:]
            brec = ar.get(key + ".brec", (nrt, 2 * cout, 2))
            pair = (dcur, dcur.stride(0), out, out.stride(0), tz, tz.stride(0), st3.all, res_z, res_z.stride(0), st_r.all, rows, cout, brec)
            hip.call("gcn_bn_bwd_reduce", *pair)
            hip.call("gcn_bn_bwd_apply", *pair, G(blk.tcn["3"].weight), G(blk.tcn["3"].bias), dtz, dtz.stride(0),
                     G(blk.residual["1"].weight), G(blk.residual["1"].bias), drz, drz.stride(0))
            y0, ymix = ar.get(key + ".y0", (rows, cout)), ar.get(key + ".ymix", (rows, cout))
            dy0 = ar.get(key + ".dy0", (rows, cout))
            wp = ar.get(key + ".wp", (2, blk.tcn["2"].weight.numel()))
            nsp = hip.lib().mmego_tconv_wgrad_nsplit(B, T, V, cout, cout, blk.taps)
            wws = ar.get("slab." + key + ".tw", (nsp * blk.taps * cout * cout,))
            hip.call("tconv_wgrad", dtz, cout, y0, cout, wws, G(blk.tcn["2"].weight), 2, B, T, V, cout, cout, blk.taps)
            slabs.add(wws, G(blk.tcn["2"].weight), 1, nsp, blk.taps * cout, cout, taps=blk.taps)
            sq = getattr(self, "_tconv_seq", [False] * 3)[i]
            nbw = B if sq else nrt
            bwrec = ar.get(key + ".bwrec", (nbw, cout, 2))
            hip.call("tconv_seq_bwd" if sq else "tconv_bwd_stats", dtz, cout, wp[1], dy0, cout, ymix, cout, st0.all, bwrec, B, T, V, cout, cout,
                     blk.taps)
            nda = hip.lib().mmego_graph_dA_fused_nblk(F)
            dAp = ar.get("slab." + key + ".dAp", (nda, K * V * V))
            hip.call("graph_dA_fused", z, z.stride(0), dy0, ymix, st0.all, bwrec, nbw, G(blk.tcn["0"].weight), G(blk.tcn["0"].bias),
                     F, V, K, cout, dAp, gcn.A, gcn.edge_importance[i], dz, dz.stride(0))
            slabs.add(dAp, G(gcn.edge_importance[i]), 2, nda, 1, K * V * V, scale=gcn.A)
            dinp = ar.get(key + ".dinp", (rows, cin))
            Wc = ops.stacked(blk.gcn.conv.weight.view(K * cout, cin), blk.residual["0"].weight.view(cout, cin))
            gWc = ops.stacked(G(blk.gcn.conv.weight).view(K * cout, cin), G(blk.residual["0"].weight).view(cout, cin))
            gbc = ops.stacked(G(blk.gcn.conv.bias), G(blk.residual["0"].bias))
            ops.grad_weight_deferred(dzr, inp, gWc, slabs, ar, "slab." + key + ".w", db=gbc)
            ops.grad_input(dzr, Wc, dinp)
            dcur = dinp
        # data_bn: only its parameter gradients (its input, the predicted skeleton, is detached: Train_Lower.py:196) ...
        dinp = dcur
        up = ar.get("up", (F, V * 3))
        st = ops.BnState(ar, "gcn.dbn", V * 3)
        hip.call("bn_param_grads", dinp.view(F, V * 3), V * 3, up, V * 3, st.all, F, V * 3, G(gcn.data_bn.weight), G(gcn.data_bn.bias))
        if input_grad:
            # ... unless somebody differentiates the skeleton: the two parameter gradients are the column sums its input gradient needs
            dup = ar.get("gcn.dup", (F, V * 3))
            hip.call("bn_input_grad", dinp.view(F, V * 3), V * 3, up, V * 3, st.all, F, V * 3, G(gcn.data_bn.weight), G(gcn.data_bn.bias),
                     dup, dup.stride(0))

    def _gcn_backward(self, ar, dk, B, T, G):
        gcn = self.keyEncoder.gcn
        V = JOINTS_UPPER
        F, rows = B * T, B * T * V
        dfz = ar.get("gcn.dfz", (rows, 64))
        hip.call("transpose_batched", dk, dfz, B, 64, T * V)      # (B,64,T*V) -> (B,T*V,64)
        cur = ar.get("gcn.b2.out", (rows, 128))
        dcur = ar.get("gcn.d3", (rows, 128))
        blocks.linear_backward(dfz, cur, gcn.fcn, G, dcur)
        for i in (2, 1, 0):
            blk = gcn.gcn_networks[i]
            cin, cout, K = blk.cin, blk.cout, blk.K
            key = "gcn.b%d" % i
            inp = ar.get("gcn.b%d.out" % (i - 1), (rows, cin)) if i > 0 else ar.get("gcn.x0", (F, V * 3)).view(rows, 3)
            out, tz = ar.get(key + ".out", (rows, cout)), ar.get(key + ".tz", (rows, cout))
            zr = ar.get(key + ".zr", (rows, (K + 1) * cout))
            z, res_z = zr[:, :K * cout], zr[:, K * cout:]
            st3, st_r, st0 = ops.BnState(ar, key + ".bn3", cout), ops.BnState(ar, key + ".bnr", cout), ops.BnState(ar, key + ".bn0", cout)
            dtz = ar.get(key + ".dtz", (rows, cout))
            dzr = ar.get(key + ".dzr", (rows, (K + 1) * cout))           # [dz | drz]: gradients of the stacked product's output
            dz, drz = dzr[:, :K * cout], dzr[:, K * cout:]
            # out = relu(BN3(tz) + BNr(res_z)): both BatchNorm backwards share dcur and the mask -- one set of launches
            ops.bn_backward_pair(dcur, out, tz, st3, G(blk.tcn["3"].weight), G(blk.tcn["3"].bias), dtz,
                                 res_z, st_r, G(blk.residual["1"].weight), G(blk.residual["1"].bias), drz)
            y0, ymix = ar.get(key + ".y0", (rows, cout)), ar.get(key + ".ymix", (rows, cout))
            # temporal convolution: weight gradient from dtz and the shifted rows of y0 (no bias gradient: a batch-statistics
            # BatchNorm follows), input gradient = the same implicit convolution of dtz on the reversed, transposed pack
            dy0 = ar.get(key + ".dy0", (rows, cout))
            wp = ar.get(key + ".wp", (2, blk.tcn["2"].weight.numel()))
            nsp = hip.lib().mmego_tconv_wgrad_nsplit(B, T, V, cout, cout, blk.taps)
            hip.call("tconv_wgrad", dtz, cout, y0, cout, ops.scratch(dtz.device, nsp * blk.taps * cout * cout), G(blk.tcn["2"].weight), 0,
                     B, T, V, cout, cout, blk.taps)
            hip.call("tconv", dtz, cout, None, wp[1], None, dy0, cout, None, B, T, V, cout, cout, blk.taps)
            dymix = ar.get(key + ".dymix", (rows, cout))
            ops.bn_backward(dy0, y0, ymix, st0, G(blk.tcn["0"].weight), G(blk.tcn["0"].bias), dymix)
            dAp = ar.get(key + ".dAp", (hip.lib().mmego_graph_dA_nblk(F), K * V * V))
            # both gradients of the einsum from one launch: dA partials and dz_k[v] = sum_w (A.imp)[k,v,w] dy[w]
            hip.call("graph_dA", z, dymix, F, V, K, cout, dAp, gcn.A, gcn.edge_importance[i], dz, z.stride(0), dz.stride(0))
            if dAp.shape[0] <= 1024 and gcn.A.is_contiguous():      # d(importance) = A . sum of the partials, one launch
                ops.colsum(dAp, G(gcn.edge_importance[i]).view(-1), scale=gcn.A.view(-1))
            else:
                dA = ar.get(key + ".dA", (K, V, V))
                ops.colsum(dAp, dA.view(-1))
                hip.call("mul", dA, gcn.A, G(gcn.edge_importance[i]), dA.numel())
            dinp = ar.get(key + ".dinp", (rows, cin))
            Wc = ops.stacked(blk.gcn.conv.weight.view(K * cout, cin), blk.residual["0"].weight.view(cout, cin))
            gWc = ops.stacked(G(blk.gcn.conv.weight).view(K * cout, cin), G(blk.residual["0"].weight).view(cout, cin))
            gbc = ops.stacked(G(blk.gcn.conv.bias), G(blk.residual["0"].bias))
            if Wc is not None and gWc is not None and gbc is not None:
                # the stacked product's gradients: one weight-gradient product (bias sums beside it) and one input-gradient
                # product for both convolutions.  (The residual conv's bias feeds a batch-statistics BatchNorm: its true gradient
                # is exactly zero and what lands in its slot is rounding noise, as in the reference's autograd.)
                ops.grad_weight(dzr, inp, gWc, db=gbc, prefer_fused=True)
                ops.grad_input(dzr, Wc, dinp)
            else:
                blocks.linear_backward(dz, inp, blk.gcn.conv, G, dinp)
                blocks.linear_backward(drz, inp, blk.residual["0"], G, dinp, accumulate_dx=True, bias_grad=False)
            dcur = dinp
        up = ar.get("up", (F, V * 3))
        st = ops.BnState(ar, "gcn.dbn", V * 3)
        scratch = ar.get("gcn.dup", (F, V * 3))
        ops.bn_backward(dcur.view(F, V * 3), None, up, st, G(gcn.data_bn.weight), G(gcn.data_bn.bias), scratch)


# =====================================================================================================
# IMU_Net (forward; it is frozen in stages 2/3 -- reference Train_Upper.py:57,136; Train_Lower.py:67,157)
# =====================================================================================================
class IMUNet(_NetBase):
    """IMUNet(input_n, output_n, hidden_n, n_rnn_layer, bidirectional=True, dropout=0);
    forward(imu[B,T,S,input_n], h0_i=None) -> (R[B,T,3,3], t[B,T,3])."""

    def __init__(self, input_n, output_n, hidden_n, n_rnn_layer, bidirectional=True, dropout=0):
        super().__init__()
        if not bidirectional or output_n != 9 or hidden_n % 32 != 0:
            raise ValueError("IMUNet HIP path supports bidirectional nets with output_n == 9 and hidden_n % 32 == 0")
        d = 2
        self.hidden_n = hidden_n
        self.fc1 = nn.Linear(input_n, hidden_n)
        self.fc2 = nn.Linear(hidden_n * d, output_n)
        self.fc3 = nn.Linear(output_n, 3)                # Q7: present in checkpoints, unused
        self.rnn_fast = LstmParams(hidden_n, hidden_n, n_rnn_layer, dropout=dropout, bidirectional=True)
        self.rnn_slow = LstmParams(2 * hidden_n, hidden_n, n_rnn_layer, dropout=dropout, bidirectional=True)
        self.attn = nn.Linear(hidden_n * d, 1)
        # "fp32" (default, the parity path) or "bf16": eval-mode BiLSTM products with bf16 operands and fp32 accumulation
        # (BASELINE config 5); everything else -- gates, cell state, pooling, heads -- stays fp32 in both modes.
        self.precision = os.environ.get("MMEGO_IMU_PRECISION", "fp32")
        # stage-1 TRAINING (imu_train.py): "split3" runs rnn_fast's input-projection, input-gradient AND weight-gradient products as
        # fp32-accurate piece products on the bf16 matrix pipe (opt-in; the recurrent steps stay on the fp32 kernels)
        self.train_precision = os.environ.get("MMEGO_IMU_TRAIN_PRECISION", "fp32")
        # what the last training forward (imu_train.forward_train) leaves for its backward: the minibatch shape, and per stack the
        # inter-layer dropout it APPLIED -- (rate, seed word, first salt) or None for rnn_fast and rnn_slow.  Backward regenerates the
        # forward's masks from this, whatever lstm_dropout or the mode have become in between.
        self._saved = None
        self._drop = (None, None)

    def _pulled_pairs(self):
        """The two directions' input weights of every BiLSTM layer back to back: stage-1 training's input gradient of a layer is
        then ONE product dgates [rows, 8H] . [W_ih ; W_ih_reverse] (imu_train.lstm_steps_backward)."""
        pulled = super()._pulled_pairs()
        for mname in ("rnn_fast", "rnn_slow"):
            for l in range(getattr(self, mname).num_layers):
                pulled["%s.weight_ih_l%d" % (mname, l)] = "%s.weight_ih_l%d_reverse" % (mname, l)
        return pulled

    def never_trained(self):
        """Q7: fc3 is in the state_dict but not in forward, so its .grad stays None in the reference and torch's Adam never
        touches it (params.FusedAdam leaves these ranges alone, weight decay included)."""
        return (self.fc3.weight, self.fc3.bias)

    def weights_changed(self):
        super().weights_changed()                  # weights may change: drop the bf16 copies of the LSTM weights
        for m in (self.rnn_fast, self.rnn_slow):
            m._bf16_cache = m._bf16_fused_cache = m._split3_cache = None

    def _forward_split3(self, ar, imu, B, T, S, Cin, H):
        """precision = "split3" (split3.hip): the fp32 forward with rnn_fast's products -- input projections and recurrent steps,
        94 % of the model's FLOPs -- on exactly split bf16 operands (a = a1 + a2 + a3, six piece products, fp32 accumulation:
        fp32-accurate at 6/16 of the fp32 matrix time).  fc1 writes the layer-0 operand itself; rnn_slow's input projections run on split operands too, its
        recurrence (64 rows: a persistent fp32 launch per layer, latency-bound, not matrix-bound), attention pooling, fc2 and the
        head are the fp32 path's kernels."""
        Bn = B * T
        dev = imu.device
        if not (H in (256, 512, 1024) and Cin <= 16 and Bn <= 2048 and self.fc1.weight.is_contiguous()):
            raise ValueError("IMUNet.precision = 'split3' needs hidden_n in (256, 512, 1024), input_n <= 16 and B*T <= 2048")
        Bp = (Bn + 31) // 32 * 32
        xf = blocks.split3_buffer(ar, "fast.x", S * Bp, H)
        hip.call("split3_fc_relu", imu.view(Bn * S, Cin), Cin, self.fc1.weight, self.fc1.bias, Bn, S, Cin, H, xf, Bp, 1)
        fast = blocks.lstm_steps_forward_split3(ar, "fast", self.rnn_fast, None, Bn, S, xfrag=xf)
        pooled = ar.get("pooled", (Bn, 2 * H))
        attn = ar.get("attn", (Bn, S))
        blocks.attn_pool_forward(fast, self.attn, Bn, S, 2 * H, pooled, attn)
        slow = blocks.lstm_steps_forward_split3_proj(ar, "slow", self.rnn_slow, pooled, B, T)
        R = torch.empty((B, T, 3, 3), dtype=torch.float32, device=dev)
        t = torch.empty((B, T, 3), dtype=torch.float32, device=dev)
        if slow.shape[1] % 256 == 0 and slow.stride(0) % 4 == 0 and slow.stride(1) == 1 and self.fc2.weight.is_contiguous():
            hip.call("imu_fc2_head", slow, slow.stride(0), self.fc2.weight, self.fc2.bias, Bn, slow.shape[1], None, R, t)
        else:
            y = ar.get("y", (Bn, 9))
            ops.linear(slow, self.fc2.weight, self.fc2.bias, y)
            hip.call("imu_head", y, Bn, R, t)
        return R, t

    def forward(self, imu, h0_i=None):
        _require_gpu(imu, "IMUNet")
        if h0_i is not None:
            raise NotImplementedError("IMUNet: the reference never passes h0_i; only None is supported")
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            from .imu_train import ImuBridge
            self.flat()
            return ImuBridge.apply(self, _f32c(imu), *self._flat.params)
        self.flat()
        ar = self.arena("eval")
        imu = _f32c(imu)
        B, T, S, Cin = imu.shape
        H = self.hidden_n
        Bn = B * T
        dev = imu.device
        if self.precision not in ("fp32", "bf16", "split3"):
            raise ValueError("IMUNet.precision must be 'fp32', 'bf16' or 'split3', got %r" % (self.precision,))
        bf16 = self.precision == "bf16"
        if self.precision == "split3":
            return self._forward_split3(ar, imu, B, T, S, Cin, H)
        if (bf16 and Bn >= blocks.FUSED_MIN_ROWS and H % 64 == 0 and Cin <= 16 and imu.is_contiguous()
                and self.fc1.weight.is_contiguous() and _BF16_FUSED_FC1):
            # large batch in the bf16 mode: fc1 + ReLU written straight as the fused step's layer-0 operand (bf16, fragment-major);
            # the fp32 activation [Bn*S, H] (1.3 GB at config 5) is never stored
            xf, Bp = blocks.fused_input_fragments(ar, "fast", Bn, S, H)
            hip.call("fc_relu_bf16_frag_tm", imu.view(Bn * S, Cin), Cin, self.fc1.weight, self.fc1.bias, Bn, S, Cin, H, xf, Bp, 1)
            # (the attention pooling behind rnn_fast reads the last layer's bf16 fragments: no fp32 h_t is stored either)
            pooled = ar.get("pooled", (Bn, 2 * H))
            attn = ar.get("attn", (Bn, S))
            fast = blocks.lstm_steps_forward_bf16_fused(ar, "fast", self.rnn_fast, None, Bn, S, xfrag=xf, pool=(self.attn, pooled, attn))
        else:
            h = ar.get("fc1", (Bn * S, H))
            ops.linear(imu.view(Bn * S, Cin), self.fc1.weight, self.fc1.bias, h, relu=True)
            if bf16:
                fast = blocks.lstm_steps_forward_bf16(ar, "fast", self.rnn_fast, h, Bn, S)
            else:
                fast = blocks.lstm_steps_forward(ar, "fast", self.rnn_fast, h, Bn, S)          # [Bn*S, 2H]
        if fast is not None:
            pooled = ar.get("pooled", (Bn, 2 * H))
            attn = ar.get("attn", (Bn, S))
            blocks.attn_pool_forward(fast, self.attn, Bn, S, 2 * H, pooled, attn)
        if bf16:
            slow = blocks.lstm_steps_forward_bf16(ar, "slow", self.rnn_slow, pooled, B, T)
        else:
            slow = blocks.lstm_steps_forward(ar, "slow", self.rnn_slow, pooled, B, T)       # [B*T, 2H]
        R = torch.empty((B, T, 3, 3), dtype=torch.float32, device=dev)
        t = torch.empty((B, T, 3), dtype=torch.float32, device=dev)
        if slow.shape[1] % 256 == 0 and slow.stride(0) % 4 == 0 and slow.stride(1) == 1 and self.fc2.weight.is_contiguous():
            # fc2 (2H -> 9) as row-wise dot products with the head behind them, one launch
            hip.call("imu_fc2_head", slow, slow.stride(0), self.fc2.weight, self.fc2.bias, Bn, slow.shape[1], None, R, t)
        else:
            y = ar.get("y", (Bn, 9))
            ops.linear(slow, self.fc2.weight, self.fc2.bias, y)
            hip.call("imu_head", y, Bn, R, t)
        return R, t
