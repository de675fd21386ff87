"""Stage trainers and the `--infer` evaluator on the HIP path.

Counterparts of the reference's Processor/Train/Train_Upper.py:20-251, Train_Lower.py:23-332,
Train_IMU.py:38-185 and Processor/Test/Demo_test.py:23-184: same class shape (``MMEgo`` with
train_upper / train_lower / train_once / eval_model), same directory side effects
(Processor/Train/{report,model,lossAndacc}/<Idx>/, log-loss.txt, log-eval.txt, epoch*_batch*frame*lr*.pth),
same stdout lines for `--infer`.  Plotting (matplotlib/seaborn) is out of scope.

Data parallel (not in the reference): when launched under torch.distributed.run each rank trains on its
own shard of every epoch's shuffled order; gradients are summed with one RCCL all-reduce per step.
"""
import contextlib
import os
import types

import numpy as np
import torch

from . import blocks, dense, hip, ops
from .config import RENDER_FPS, RENDER_SIZE, Config, ConfigDemo
from .data import DeviceArrays, FrameStore, PosePC, batch_indices
from .dense import dense_infer
from .evaluation import (BREAKDOWN_BINS, METRICS, PCK_THRESHOLDS_CM, Breakdown, _jitter_imu, _jitter_pose, aligned_summary, check_breakdown,
                         dataset_groups, imu_noise_key, imu_noise_line, imu_noise_of, pose_noise_key, pose_noise_line, pose_noise_of,
                         print_aligned, print_breakdown, print_reference)
from .nets import IMUNet, LowerNet, UpperNet
from .params import FusedAdam, LrSchedule, describe_decay, lr_schedule_of, resolve_no_decay
from .nets_local import UpperNetwlocal
from .train_step import TRAINED, ImuStep, PipelinedStages, StageStep, broadcast_flag, call_upper, empty_step, shard_of, sync_replicas
from .utils import EarlyStopping

_HERE = os.path.dirname(os.path.abspath(__file__))
# where report/, model/, lossAndacc/ go: the reference's Processor/Train (Train_Upper.py:22-50) unless MMEGO_TRAIN_DIR says otherwise
_TRAIN_DIR = os.environ.get("MMEGO_TRAIN_DIR") or os.path.join(os.path.dirname(_HERE), "Processor", "Train")


UPPER_VARIANTS = {"global": UpperNet, "wlocal": UpperNetwlocal}          # --upper_variant -> the class behind "Upper_Net"


def upper_variant_of(state_dict):
    """Which Upper net a state_dict belongs to, by its keys (the anchor branch and its combine head against the plain head); None: neither."""
    keys = list(state_dict)
    if any(k.startswith(("module2.", "module3.")) for k in keys):
        return "wlocal"
    if any(k.startswith("mlpHead.") for k in keys):
        return "global"
    return None


def load_upper_state(net, state_dict, variant, source):
    """load_state_dict for an Upper net built for --upper_variant ``variant``: a checkpoint of the other variant ends the run with a message
    that names the flag instead of a list of mismatched keys."""
    found = upper_variant_of(state_dict)
    if found is not None and found != variant:
        raise SystemExit("%s is an Upper_Net checkpoint of the %r variant (%s), but this run builds the %r variant (%s): pass "
                         "--upper_variant %s, or a checkpoint of the %r variant"
                         % (source, found, UPPER_VARIANTS[found].__name__, variant, UPPER_VARIANTS[variant].__name__, found, variant))
    net.load_state_dict(state_dict)


class _Base:
    """Shared set-up: directories, frozen IMU_Net (or ground-truth head pose), datasets."""
    finetune_imu = False          # (--finetune_imu: set by the stage trainers from the config)
    finetune_upper = False        # (--finetune_upper: likewise)
    pose_noise = None             # (--pose_noise_deg, --pose_noise_t: (deg, t, seed), set by the stage trainers from the config)
    imu_noise = None              # (--imu_noise_*, --imu_bias_*: (six sigmas, seed), set by the trainers from the config)
    # The trainer's optimisers, keyed like train_step.TRAINED ("opt": the stage's own net, "imu_opt", "upper_opt"): ONE set, handed to
    # the step of every minibatch size, read by the grad-norm report and the checkpoint (a trainer's __init__ makes it a dict)
    _opts = types.MappingProxyType({})
    _resume = None                # (the train state --resume loaded: load_train_state; a trainer's __init__ starts it as None too)
    weight_decay = 0.0            # of "opt" (stage 1: coupled 1e-3)
    last_metrics = None           # (--metrics full: aligned_summary of the last evaluation pass; eval_model's return value stays the reference's)
    net_name = None               # what "opt" trains, as the grad-norm report calls it

    def __init__(self, cfg, make_dirs=True):
        self.cfg = cfg
        self.device = torch.device(cfg.device)
        if self.device.type != "cuda":
            raise RuntimeError("the mmego_amd processors run on the MI355X HIP path only (device=%s)" % cfg.device)
        hip.lib()
        self.frame_no, self.batchsize = cfg.frame_no, getattr(cfg, "batch_size", 20)
        self.Idx = cfg.Idx
        self.world = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
        self.rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        self.pg = torch.distributed.group.WORLD if self.world > 1 else None
        if make_dirs and self.rank == 0:
            for sub in ("report", "model", "lossAndacc"):
                path = os.path.join(_TRAIN_DIR, sub, str(self.Idx))
                os.makedirs(path, exist_ok=True)
                print("%s saved in %s" % ({"report": "report", "model": "model", "lossAndacc": "Loss and accuracy"}[sub], path))

    def _dp_start(self, model):
        """Data parallel: every replica starts from rank 0's weights and buffers (the nets are built from each rank's own
        torch RNG unless --seed is given), and the dropout streams of the ranks are decorrelated (SURVEY 8-e ii)."""
        if self.world > 1:
            sync_replicas(model, self.pg)
            model.seed_counter().bitwise_xor_((self.rank * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF)

    def _frame_store_options(self):
        """(--window_jitter, --point_keep, (--point_noise, --point_noise_v)): any of them makes the training split a data.FrameStore
        instead of DeviceArrays."""
        keep, noise = getattr(self.cfg, "point_keep", None), [getattr(self.cfg, k, None) for k in ("point_noise", "point_noise_v")]
        return (bool(getattr(self.cfg, "window_jitter", False)), None if keep is None else float(keep),
                tuple(None if v is None else float(v) for v in noise))

    def _load_splits(self):
        """The two PosePC splits; the training one keeps its per-frame clouds when a FrameStore is going to serve it."""
        jitter, keep, noise = self._frame_store_options()
        self.train_data = PosePC(batch_length=self.frame_no, keep_frames=jitter or keep is not None or noise != (None, None))
        self.test_data = PosePC(train=False, batch_length=self.frame_no)
        self._epoch = 0               # (the epoch _epochs is in: what a FrameStore draws its window starts and packing seeds from)

    def _train_arrays(self):
        """The training split in HBM, uploaded at the first training pass: finished windows (DeviceArrays: the reference's windows, the
        loader's packing), or -- --window_jitter / --point_keep / --point_noise / --point_noise_v -- frames (FrameStore), told which epoch begins."""
        if self._train_dev is None:
            jitter, keep, noise = self._frame_store_options()
            if not jitter and keep is None and noise == (None, None):
                self._train_dev = DeviceArrays(self.train_data, self.device)
            else:
                fs = self._train_dev = FrameStore(self.train_data, self.device, jitter=jitter, point_keep=keep,
                                                  seed=getattr(self.cfg, "seed", None) or 0, point_noise=noise[0], point_noise_v=noise[1])
                if self.rank == 0:
                    said = "" if keep is None else "; clouds re-drawn per minibatch, point_keep %g" % keep
                    if noise != (None, None):
                        said += "%s; return noise sigma %s" % ("; clouds re-drawn per minibatch" if keep is None else "", ", ".join(
                            "%s %g" % (n, v) for n, v in zip(("xyz", "velocity"), noise) if v is not None))
                    print("[mmego_amd] frame store: %d frames, %d valid window starts (%d training windows, %d of them movable)%s%s"
                          % (fs.F, len(fs.valid_starts()), fs.n, fs.n_movable, "; window jitter on" if jitter else "", said))
        if isinstance(self._train_dev, FrameStore):
            self._train_dev.begin_epoch(self._epoch)
        return self._train_dev

    def _log_mode(self):
        return "a" if getattr(self.cfg, "resume_path", None) else "w"     # --resume continues the logs instead of truncating them

    def _upper_variant(self):
        v = getattr(self.cfg, "upper_variant", None) or "global"
        if v not in UPPER_VARIANTS:
            raise SystemExit("--upper_variant: %r is not one of %s" % (v, ", ".join(sorted(UPPER_VARIANTS))))
        return v

    def _metrics(self):
        return getattr(self.cfg, "metrics", None) or "reference"

    def _new_upper(self, path=None):
        """The Upper net of --upper_variant on the device; ``path``: a checkpoint to load into it."""
        v = self._upper_variant()
        net = UPPER_VARIANTS[v]().to(self.device)
        if path is not None:
            load_upper_state(net, torch.load(path, map_location=self.device), v, path)
        return net

    def _load_imu(self):
        # (--finetune_imu, --finetune_all: built without dropout -- same state_dict keys -- as in stage 1, unless --imu_dropout asks for a rate)
        trained = getattr(self.cfg, "finetune_imu", False) or getattr(self.cfg, "finetune_all", False)
        drop = (getattr(self.cfg, "imu_dropout", None) or 0) if trained else 0.1
        imu = IMUNet(15, 6 + 3, 512, 2, True, drop).to(self.device).eval()
        if self.cfg.gt_head_pose:
            print("[mmego_amd] head pose from the recording (R_R0R, ground-truth head joint); IMU_Net not used")
            return None
        if not os.path.exists(self.cfg.model_IMU_path):
            raise FileNotFoundError("IMU_Net checkpoint %s not found (it is absent from the reference snapshot); pass "
                                    "--load_IMU_path or --gt_head_pose" % self.cfg.model_IMU_path)
        imu.load(self.cfg.model_IMU_path)
        return imu

    def head_pose(self, imu_net, imu, R_R0R, target):
        """(R, t) fed to Upper/Lower: frozen IMU_Net output, or the recorded pose when --gt_head_pose."""
        if imu_net is None:
            return R_R0R.contiguous(), target[:, :, 20].contiguous()
        with torch.no_grad():
            return imu_net(imu)

    def save_models(self, epoch, model, optimizer=None, early=None):
        """The reference's checkpoint (state_dict only, same file name: Train_Upper.py:69-74) plus, beside it, a
        `.train_state.pth` with what a bit-exact `--resume` needs and the reference never saved: Adam moments and step
        count, the epoch, the minibatch-order RNG, the dropout counter and the early-stopping state."""
        if self.rank != 0:
            return None
        path = os.path.join(_TRAIN_DIR, "model", str(self.Idx), "epoch{}_batch{}frame{}lr{}.pth".format(
            epoch, self.batchsize, self.frame_no, self.learning_rate))
        torch.save(model.state_dict(), path)
        if optimizer is not None:
            torch.save({"epoch": epoch + 1, "model": model.state_dict(), "optimizer": optimizer.state_dict(),
                        "rng": self._rng.get_state(), "dropout_counter": model.seed_counter().cpu(),
                        "early": None if early is None else (early.counter, early.best_score)},
                       path[:-4] + ".train_state.pth")
        return path

    def load_train_state(self, path, model):
        """Restore a `.train_state.pth` written by save_models (or the one beside a given model `.pth`)."""
        if not path.endswith(".train_state.pth"):
            path = path[:-4] + ".train_state.pth"
        ts = torch.load(path, map_location="cpu", weights_only=False)
        if isinstance(model, tuple(UPPER_VARIANTS.values())):
            load_upper_state(model, ts["model"], self._upper_variant(), path)
        else:
            model.load_state_dict(ts["model"])
        model.seed_counter().copy_(ts["dropout_counter"])
        self._rng.set_state(ts["rng"])
        self.start_epoch = int(ts["epoch"])
        self._resume = ts
        print("[mmego_amd] resumed from %s at epoch %d" % (path, self.start_epoch))
        return ts

    def _say_imu_noise(self):
        """The one line a training run under --imu_noise_* / --imu_bias_* prints when it starts."""
        if self.rank == 0:
            sig, seed = self.imu_noise
            print("[mmego_amd] IMU noise: white rotation %g deg per axis, accelerometer %g, gyroscope %g; bias per window rotation %g deg per "
                  "axis, accelerometer %g, gyroscope %g; re-drawn per minibatch from (seed %d, epoch, minibatch, rank); evaluation untouched"
                  % (sig + (seed,)))

    def _lr_schedule(self):
        """The run's learning-rate schedule (params.LrSchedule; None: a constant rate), worked out ONCE, ahead of the first optimiser:
        from the options, a decay without --lr_decay_steps spanning the rest of the run.  Under --resume the schedule the optimiser
        state carries wins, as lr and ema_decay do, and options that name another one end the run.  Says the start line (rank 0)."""
        if not hasattr(self, "_lr_sched"):
            sched = None
            if getattr(self.cfg, "lr_schedule", None) is not None or getattr(self.cfg, "lr_warmup", None) is not None:
                per_epoch = -(-len(self.train_data) // (self.batchsize * self.world))      # (global minibatches: the optimiser steps of an epoch)
                sched = lr_schedule_of(self.cfg, self.num_epochs, per_epoch)
            saved = None if self._resume is None else self._resume["optimizer"].get("lr_schedule")
            if self._resume is not None:
                saved = None if saved is None else LrSchedule.from_dict(saved)
                if sched is not None and sched != saved:
                    raise SystemExit("--resume: the training state was saved under %s, and the --lr_* options name %r: leave them out (the "
                                     "saved schedule is continued) or start a new run"
                                     % ("no learning-rate schedule" if saved is None else "the learning-rate schedule %r" % (saved,), sched))
                sched = saved
            self._lr_sched = sched
            if sched is not None and self.rank == 0:
                print("[mmego_amd] learning-rate schedule: %s" % sched.describe())
        return self._lr_sched

    def _report_lr(self):
        """With a schedule: after an epoch's training pass, one line per trained net with the rate of its last step (one device double per
        optimiser), to stdout and log-eval.txt."""
        if self._lr_schedule() is None or self.rank != 0:
            return
        names = {"opt": self.net_name, "imu_opt": "IMU_Net", "upper_opt": "Upper_Net"}
        for o, _ in TRAINED:
            if o in self._opts and self._opts[o].lr_schedule is not None:
                line = "LR ({}): {:.9g}".format(names[o], self._opts[o].current_lr())
                print(line)
                if getattr(self, "evalfile", None) is not None:
                    self.evalfile.write(line + "\n")
                    self.evalfile.flush()

    def _decay_options(self):
        """--weight_decay / --decay_mode / --no_decay_1d as (W or None: the reference's decays, FusedAdam's decoupled, its no_decay)."""
        w = getattr(self.cfg, "weight_decay", None)
        if w is None:
            return None, False, None
        return float(w), getattr(self.cfg, "decay_mode", None) == "adamw", "1d" if getattr(self.cfg, "no_decay_1d", False) else None

    def _say_decay(self):
        """Under the decay options (or a resumed state that carries them): one line per trained net, once, when its optimisers exist."""
        opts = [(o, self._opts[o]) for o, _ in TRAINED if o in self._opts]
        if getattr(self, "_decay_said", False) or not opts:
            return
        self._decay_said = True
        if self._decay_options()[0] is None and not any(opt.decoupled or opt.no_decay for _, opt in opts):
            return
        names = {"opt": self.net_name, "imu_opt": "IMU_Net", "upper_opt": "Upper_Net"}
        for o, opt in opts:
            if self.rank == 0:
                tensors, elements = opt.decay_counts()
                print("[mmego_amd] weight decay (%s): %s, W %g; %d of %d tensors and %d of %d elements decay"
                      % (names[o], "adamw" if opt.decoupled else "l2", opt.weight_decay, tensors, len(opt.flat.params), elements,
                         sum(p.numel() for p in opt.flat.params)))

    def _main_opt(self, model):
        """The optimiser of the trainer's own net: built ONCE -- by the first step or the first empty-shard step, whichever comes -- and
        that is where a --resume state is loaded."""
        if "opt" not in self._opts:
            w, decoupled, no_decay = self._decay_options()
            opt = self._opts["opt"] = FusedAdam(model.flat(), lr=self.learning_rate, weight_decay=self.weight_decay if w is None else w,
                                                max_grad_norm=getattr(self.cfg, "clip_grad_norm", None), ema_decay=getattr(self.cfg, "ema_decay", None),
                                                lr_schedule=self._lr_schedule(), decoupled=decoupled, no_decay=no_decay)
            if self._resume is not None:
                self._check_resumed_decay(model)
                opt.load_state_dict(self._resume["optimizer"])
        return self._opts["opt"]

    def _check_resumed_decay(self, model):
        """--resume: the saved decay is continued without the flags, as lr and ema_decay are; flags that name another one end the run."""
        w, decoupled, no_decay = self._decay_options()
        if w is None or self._resume is None:
            return
        sd = self._resume["optimizer"]
        saved = (float(sd["weight_decay"]), bool(sd.get("decoupled", False)), tuple(sorted(sd.get("no_decay") or ())))
        named = (w, decoupled, resolve_no_decay(model, no_decay))
        if saved != named:
            raise SystemExit("--resume: the training state was saved under the weight decay [W %g, %s], and the --weight_decay / --decay_mode "
                             "/ --no_decay_1d options name [W %g, %s]: leave them out (the saved setting is continued) or start a new run"
                             % (saved[0], describe_decay(*saved[1:]), named[0], describe_decay(*named[1:])))

    def save_beside(self, epoch, folder, net, state_dict=None):
        """A second trained net beside the stage's checkpoint, same file name, in a folder of its own (--finetune_imu: IMU_Net,
        --finetune_upper: Upper_Net, --finetune_all: both); ``state_dict``: written instead of ``net``'s own (--ema_decay: the averaged
        weights, under EMA/)."""
        if self.rank != 0:
            return None
        folder = os.path.join(_TRAIN_DIR, "model", str(self.Idx), folder)
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, "epoch{}_batch{}frame{}lr{}.pth".format(epoch, self.batchsize, self.frame_no, self.learning_rate))
        torch.save(net.state_dict() if state_dict is None else state_dict, path)
        return path

    def _averaging(self):
        """[(optimiser key, optimiser)] of the trainer's optimisers that keep a weight average (--ema_decay, or a resumed state's)."""
        return [(o, self._opts[o]) for o, _ in TRAINED if o in self._opts and self._opts[o].ema_decay is not None]

    def _save_averaged(self, epoch, model, also_saved):
        """--ema_decay: beside every file just saved, the same net with its averaged weights (FusedAdam.ema_state_dict: reference format,
        loads wherever the raw file loads) under the same name in EMA/ -- EMA/IMU_Net/, EMA/Upper_Net/ for the nets saved beside."""
        if self.rank != 0:
            return
        opts = dict(self._averaging())
        targets = [("opt", "EMA", model)] + [({"IMU_Net": "imu_opt", "Upper_Net": "upper_opt"}[folder], "EMA/" + folder, net)
                                             for folder, net in also_saved]
        for key, folder, net in targets:
            if key in opts:
                self.save_beside(epoch, folder, net, state_dict=opts[key].ema_state_dict())

    def _epochs(self, model, train, evaluate, report, also_saved=()):
        """The epoch loop of every trainer (reference Train_Upper.py:90-132, Train_Lower.py:110-153, Train_IMU.py:90-112).  ``train()``: one
        training pass; ``evaluate()`` -> a tuple that starts (eval_loss, eval_loss_l, ...); ``report(epoch, what train() returned, what
        evaluate() returned)``: the trainer's lines beyond log-loss.txt, called on every rank; ``also_saved``: (folder, net) pairs
        saved beside the checkpoint."""
        early = EarlyStopping(patience=30)
        if getattr(self.cfg, "resume_path", None):
            ts = self.load_train_state(self.cfg.resume_path, model)
            if ts["early"] is not None:
                early.counter, early.best_score = ts["early"]
        # --ema_decay (a resumed run: the decay its optimiser state carries, the flag need not be repeated)
        decay = getattr(self.cfg, "ema_decay", None)
        if self._resume is not None and self._resume["optimizer"].get("ema_decay") is not None:
            decay = self._resume["optimizer"]["ema_decay"]
        if decay is not None and self.rank == 0:
            print("[mmego_amd] weight averaging: decay %g; evaluation and early stopping use the averaged weights" % decay)
        self._lr_schedule()                                        # (the start line, and a refusal, ahead of the first epoch)
        self._check_resumed_decay(model)                           # (likewise a refusal)
        out = None
        names = {"opt": self.net_name, "imu_opt": "IMU_Net", "upper_opt": "Upper_Net"}
        for epoch in range(self.start_epoch, self.num_epochs):
            print("epoch: {}".format(epoch + 1))
            self._epoch = epoch
            trained = train()
            report_grad_norms(self.rank, [(names[o], self._opts[o]) for o, _ in TRAINED if o in self._opts])
            self._report_lr()
            # a persistent rnn_slow launch of the frozen IMU_Net whose workgroups were not co-resident reports it only through a
            # sticky word: read once per epoch (the training pass has just synchronised for its log) -- never train on silently
            blocks.seq_xcd_raise()
            sync_replicas(model, self.pg, params=False)            # BatchNorm running statistics: rank 0's, on every rank
            # (--ema_decay: the evaluation pass -- the report, model selection and early stopping with it -- runs on every trained net's
            #  averaged weights; the contents are exchanged back, bit for bit, before anything is saved or trained further)
            with contextlib.ExitStack() as averaged:
                for _, opt in self._averaging():
                    averaged.enter_context(opt.averaged())
                out = evaluate()
            eval_loss, eval_loss_l = out[0], out[1]
            if self.rank == 0:
                self.lossfile.write("%d %f\n" % (epoch + 1, eval_loss))
                self.lossfile.write(str(eval_loss_l) + "\n")
                self.lossfile.flush()
            report(epoch, trained, out)
            # every rank evaluates its own copy of the test split (the reference's unseeded padding makes them differ), so
            # the ranks could disagree on when to stop and leave each other hanging in the next all-reduce: rank 0 decides
            stop = broadcast_flag(early(eval_loss), self.device, self.pg)
            # (the reference saves before the evaluation pass; saving after it keeps the RNG / early-stopping state in the
            #  checkpoint consistent with "epoch finished", which is what --resume continues from)
            if (epoch + 1) % self.save_slot == 0 or epoch + 1 == self.num_epochs or stop:
                self.save_models(epoch, model, self._main_opt(model), early)
                for folder, net in also_saved:
                    self.save_beside(epoch, folder, net)
                self._save_averaged(epoch, model, also_saved)
            if stop:
                print("Early stopping")
                break
        return out

    def pose_metrics(self, upper_l, lower_l, target):
        """Demo_test per-batch figures on the device -> (all, upper, lower, per_joint[21], angle[20])."""
        F = upper_l.shape[0] * upper_l.shape[1]
        E = torch.empty((F, 43), dtype=torch.float32, device=self.device)
        hip.call("pose_errors", upper_l.contiguous(), lower_l.contiguous(), target.contiguous(), F, E)
        s = torch.empty(43, dtype=torch.float32, device=self.device)
        ops.colsum(E, s)
        m = (s / F).cpu().numpy().astype(np.float64)
        return float(m[:21].mean()), float(m[41]), float(m[42]), m[:21], m[21:41]


def report_grad_norms(rank, named_opts):
    """--clip_grad_norm: after an epoch's training pass, one line per trained net from ONE device read per optimiser (rank 0), then the
    counters start again.  An optimiser that does not clip (no flag) is neither read nor reported."""
    for name, opt in named_opts:
        if opt is None or opt.max_grad_norm is None:
            continue
        if rank == 0:
            s = opt.grad_stats()
            print("Grad norm ({}): mean {:.6g} max {:.6g} clipped {}/{} skipped {}".format(
                name, s["mean"], s["max"], s["clipped"], s["steps"], s["skipped"]))
        opt.reset_grad_stats()


class _StageTrainer(_Base):
    stage = None

    def __init__(self):
        super().__init__(Config)
        cfg = self.cfg
        self.num_epochs, self.save_slot, self.learning_rate = cfg.epochs, 50, cfg.lr
        self.finetune_all = bool(getattr(cfg, "finetune_all", False))
        if self.finetune_all and (self.stage != "lower" or cfg.gt_head_pose or self.world > 1 or getattr(cfg, "resume_path", None)
                                  or getattr(cfg, "finetune_imu", False) or getattr(cfg, "finetune_upper", False)):
            raise SystemExit("--finetune_all: Lower_Net stage with an IMU_Net checkpoint only, without --finetune_imu / --finetune_upper; not "
                             "data parallel, not with --resume")
        # (--finetune_all: the Lower stage with both options -- train_step.StageStep's three-net step)
        self.finetune_imu = bool(getattr(cfg, "finetune_imu", False)) or self.finetune_all
        if self.finetune_imu and not self.finetune_all and (self.stage != "upper" or cfg.gt_head_pose or self.world > 1 or getattr(cfg, "resume_path", None)):
            raise SystemExit("--finetune_imu: Upper_Net stage with an IMU_Net checkpoint only; not data parallel, not with --resume")
        self.finetune_upper = bool(getattr(cfg, "finetune_upper", False)) or self.finetune_all
        if self.finetune_upper and (self.stage != "lower" or self.world > 1 or getattr(cfg, "resume_path", None)):
            raise SystemExit("--finetune_upper: Lower_Net stage only; not data parallel, not with --resume")
        if self.finetune_upper and self._upper_variant() != "global":
            raise SystemExit("--upper_variant wlocal: --finetune_upper / --finetune_all train a plain UpperNet only (UpperNetwlocal stays "
                             "frozen in stage 3)")
        self.pose_noise = pose_noise_of(cfg)                           # (--pose_noise_deg, --pose_noise_t: (deg, t, seed) or None)
        if self.pose_noise is not None:
            if self.finetune_imu:
                raise SystemExit("--pose_noise_deg / --pose_noise_t perturb a head pose that is data: not with --finetune_imu / --finetune_all, "
                                 "which train it")
            if self.rank == 0:
                print("[mmego_amd] head-pose noise: rotation %g deg per axis, translation %g m, re-drawn per minibatch from (seed %d, epoch, "
                      "minibatch, rank); evaluation untouched" % self.pose_noise)
        self.model_IMU = self._load_imu()
        self.imu_noise = imu_noise_of(cfg)                             # (--imu_noise_*, --imu_bias_*: (six sigmas, seed) or None)
        if self.imu_noise is not None:
            if self.model_IMU is None:
                raise SystemExit("--imu_noise_* / --imu_bias_* perturb what IMU_Net reads: not with --gt_head_pose, where none runs")
            self._say_imu_noise()
        self._opts = {}
        self._load_splits()
        rep = os.path.join(_TRAIN_DIR, "report", str(self.Idx))
        self.lossfile = open(os.path.join(rep, "log-loss.txt"), self._log_mode()) if self.rank == 0 else None
        self.evalfile = open(os.path.join(rep, "log-eval.txt"), self._log_mode()) if self.rank == 0 else None
        self._steps = {}
        self._rng = np.random.RandomState(1234)
        self.start_epoch, self._resume = 0, None
        self._train_dev = None
        self._log = None

    def _step_for(self, B):
        """One StageStep (static buffers, optional HIP graph) per minibatch size.  With a frozen IMU_Net in the loop its forward
        runs one minibatch ahead of the trainable body (train_step.PipelinedStages: same results bit for bit, the compute-bound
        IMU_Net forward of minibatch i+1 overlaps the latency-bound body of minibatch i); MMEGO_PIPELINE_IMU=0 turns that off."""
        st = self._steps.get(B)
        if st is None:
            pg = self.pg
            # (--finetune_imu: the plain StageStep -- the IMU_Net is trained, there is no frozen forward to run ahead)
            pipelined = (self.model_IMU is not None and not self.finetune_imu and os.environ.get("MMEGO_PIPELINE_IMU", "1") != "0")
            # (--finetune_upper: the plain StageStep too -- the engines around a frozen IMU_Net forward refuse a stage with two trained nets)
            pipelined = pipelined and not self.finetune_upper
            # (--imu_noise_* / --imu_bias_*: the plain StageStep too -- the noise launch sits in front of the stage's OWN IMU_Net forward,
            #  inside its body, and a forward that ran one minibatch ahead would have to know the NEXT minibatch's key)
            pipelined = pipelined and self.imu_noise is None
            imu_lr = getattr(self.cfg, "imu_lr", None)
            self._main_opt(self.model)
            w, decoupled, no_decay = self._decay_options()
            decay = {} if w is None else dict(weight_decay=w, imu_weight_decay=w, decoupled=decoupled, no_decay=no_decay)
            # (one optimiser state per trained net for all batch sizes: the step takes what the dict holds and adds what it builds)
            st = StageStep(self.stage, self.model, None if pipelined else self.model_IMU,
                           upper_frozen=getattr(self, "Upper_net", None), lr=self.learning_rate, process_group=pg,
                           use_graph=not pipelined, finetune_imu=self.finetune_imu,
                           imu_lr=self.learning_rate if imu_lr is None else imu_lr,
                           finetune_upper=self.finetune_upper, upper_lr=getattr(self.cfg, "upper_lr", None),
                           clip_grad_norm=getattr(self.cfg, "clip_grad_norm", None), optimisers=self._opts,
                           ema_decay=getattr(self.cfg, "ema_decay", None), lr_schedule=self._lr_schedule(),
                           **({} if self.pose_noise is None else dict(pose_noise_deg=self.pose_noise[0], pose_noise_t=self.pose_noise[1])),
                           **({} if self.imu_noise is None else dict(imu_noise=self.imu_noise[0])), **decay)
            self._say_decay()
            st.engine = None
            if pipelined:
                st.imu_next = torch.empty((B, self.frame_no) + tuple(self._train_dev.shape["imu"][1:]), dtype=torch.float32,
                                          device=self.device)
                st.engine = PipelinedStages([st], [self.model_IMU], st.imu_next, use_graph=True)
            self._steps[B] = st
        return st

    def train_once(self):
        self.model.train()
        if self.finetune_imu:
            self.model_IMU.train()                                      # (.eval() again for the epoch evaluation: eval_model)
        if self.finetune_upper:
            self.Upper_net.train()                                      # (likewise)
        nsel = self.model_out_joints
        if self._log is None:
            self._log = torch.zeros((64, 2), dtype=torch.float32, device=self.device)
        nlog, scales = 0, []
        self._train_arrays()                                            # the training set lives in HBM (51 MB for Sample_data)
        todo = [idx[shard_of(self.rank, self.world)]                    # this rank's shard of every global minibatch
                for idx in batch_indices(len(self.train_data), self.batchsize * self.world, True, self._rng)]
        primed = None                                                   # number of the minibatch whose head poses are ready
        for i, idx in enumerate(todo):
            B = len(idx)
            if B == 0:              # short last global minibatch, nothing for this rank: zero gradient, same collective + update
                empty_step(self.model, self._main_opt(self.model), self.pg)
                primed = None
                continue
            st = self._step_for(B)
            b = self._train_dev.gather(idx)                             # on-device gather into per-batch-size static buffers
            tgt = b["target"]
            if st.static is None or st.static["x_src"].data_ptr() != b["data"].data_ptr():
                st.bind(b["data"], b["imu"], b["skl"], tgt, R_gt=b["R_R0R"])
            if self.pose_noise is not None:                             # this minibatch's head-pose draw (the word the captured launch reads)
                st.set_pose_key(pose_noise_key(self.pose_noise[2], self._epoch, i, self.rank))
            if self.imu_noise is not None:                              # and its IMU draws
                st.set_imu_key(imu_noise_key(self.imu_noise[1], self._epoch, i, self.rank))
            if st.engine is None:
                st.step()
            else:
                if primed != i:                                         # first minibatch, or the size changed: no forward ran ahead
                    st.imu_next.copy_(b["imu"])
                    st.engine.prime()
                if i + 1 < len(todo) and len(todo[i + 1]) == B:         # IMU samples of the next minibatch for the forward that
                    self._train_dev.gather_field_into("imu", todo[i + 1], st.imu_next)      # runs beside this body
                    primed = i + 1
                else:
                    primed = None
                st.engine.step()
            # per-minibatch log (L1 sum, mean joint distance): kept on the device, read once per epoch (the reference
            # calls loss.item() every step: Train_Upper.py:183-186)
            if nlog == self._log.shape[0]:
                self._log = torch.cat((self._log, torch.zeros_like(self._log)))
            ops.copy2d(st.loss2.view(1, 2), self._log[nlog:nlog + 1])
            scales.append(1.0 / (B * self.frame_no * nsel))
            nlog += 1
        log = self._log[:nlog].cpu().numpy()
        losses = [float(v) for v in log[:, 0]]
        accs = [float(v * sc) for v, sc in zip(log[:, 1], scales)]
        assert nsel in (15, 8)
        return accs, losses

    def _train_loop(self, extra_print):
        """``extra_print(epoch, out)``: rank 0's lines to log-eval.txt and stdout."""
        return self._epochs(self.model, self.train_once, self.eval_model,
                            lambda epoch, _, out: extra_print(epoch, out) if self.rank == 0 else None,
                            ([("IMU_Net", self.model_IMU)] if self.finetune_imu else []) +
                            ([("Upper_Net", self.Upper_net)] if self.finetune_upper else []))


class UpperTrainer(_StageTrainer):
    """`python main.py --train --network Upper_Net` (reference Train_Upper.MMEgo)."""
    stage, net_name = "upper", "Upper_Net"
    model_out_joints = 15

    def __init__(self):
        super().__init__()
        self.model = self._new_upper(self.cfg.model_upper_path if self.cfg.Upper_pretrained else None)      # (--upper_variant)
        self._dp_start(self.model)

    def train_upper(self):
        def report(epoch, out):
            eval_loss, eval_loss_l, eval_accu, dis_l, accu_ll, angle_ll = out
            self.evalfile.write("%d %f %f\n" % (epoch + 1, eval_accu, sum(angle_ll) / len(angle_ll)))
            self.evalfile.write(str(accu_ll) + "\n" + str(angle_ll) + "\n" + str(accu_ll[self.cfg.hand_joint_map]) + "\n")
            self.evalfile.flush()
            print("\n wrist elbow(l, r): {}".format(accu_ll[self.cfg.hand_joint_map]))
            print("Average Joint Localization Error: {}".format(eval_accu))
            print("Average Joint Rotation Error: {}".format(sum(angle_ll) / len(angle_ll)))
            print(accu_ll)
            print("Eval_loss: {} Eval_loss_l (l, g): {} \n Angle_loss: {} \n".format(eval_loss, eval_loss_l, angle_ll))
            if self.last_metrics is not None:                        # (--metrics full: stdout only, the log files keep their format)
                print(metrics_line(self.last_metrics))
        return self._train_loop(report)

    def eval_model(self):
        """Reference Processor/Train/Train_Upper.py:189-251, on the device end to end: the test split lives in HBM (DeviceArrays,
        uploaded once), minibatches are gathered there, the per-frame figures come from one kernel (mmego_pose_errors_upper), their
        per-minibatch sums land in a device-side log, and the host reads that log ONCE per epoch.  Returns the reference's tuple
        (eval_loss, eval_loss_l, eval_accu, dis_l, accu_ll[15], angle_ll[14]): means over minibatches of per-minibatch means."""
        self.model.eval()
        if self.finetune_imu:
            self.model_IMU.eval()
            self.model_IMU.weights_changed()          # (the fused Adam writes through raw pointers: no derived copy of old weights)
        m = _epoch_eval(self, self.test_data, self.batchsize, True, self._rng, self.model_IMU, self.model, None, self._metrics())
        self.last_metrics = aligned_summary(m[:, 30:], 15) if self._metrics() == "full" else None      # (--metrics full: the 15 upper joints)
        eval_loss = float(np.mean(m[:, 29]))                                 # L1(sum) / B / T per minibatch
        return (eval_loss, np.asarray([eval_loss / self.cfg.joint_num_upper]), float(np.mean(m[:, :15].mean(axis=1))),
                float(np.mean(m[:, 29] / 45.0)), m[:, :15].mean(axis=0), m[:, 15:29].mean(axis=0))


class LowerTrainer(_StageTrainer):
    """`python main.py --train --network Lower_Net` (reference Train_Lower.MMEgo)."""
    stage, net_name = "lower", "Lower_Net"
    model_out_joints = 8

    def __init__(self):
        super().__init__()
        self.model = LowerNet(hidden_dim=64).to(self.device)
        if self.cfg.Lower_pretrained:
            self.model.load(self.cfg.model_lower_path)
        self.Upper_net = self._new_upper(self.cfg.model_upper_path).eval()      # (--upper_variant: the class the checkpoint is loaded into)
        self._dp_start(self.model)

    def train_lower(self):
        def report(epoch, out):
            eval_loss, eval_loss_l, eval_accu, accu_lower, accu_ll, angle_ll = out
            self.evalfile.write("%d %f %f %f\n" % (epoch + 1, eval_accu, accu_lower, sum(angle_ll) / len(angle_ll)))
            self.evalfile.write(str(accu_ll) + "\n" + str(angle_ll) + "\n" + str(accu_ll[self.cfg.hand_joint_map]) + "\n")
            self.evalfile.flush()
            print("\n wrist elbow(l, r): {}".format(accu_ll[self.cfg.hand_joint_map]))
            print("Average Joint Localization Error: {}".format(eval_accu))
            print("Average LowerBody Joint Localization Error: {}".format(accu_lower))
            print("Average Joint Rotation Error: {}".format(sum(angle_ll) / len(angle_ll)))
            print(accu_ll)
            print("Eval_loss: {} Eval_loss_l (l, g): {} \n Angle_loss: {}".format(eval_loss, eval_loss_l, angle_ll))
            if self.last_metrics is not None:                        # (--metrics full: stdout only, the log files keep their format)
                print(metrics_line(self.last_metrics))
        return self._train_loop(report)

    def eval_model(self):
        self.model.eval()
        if self.finetune_upper:
            self.Upper_net.eval()
            self.Upper_net.weights_changed()          # (the fused Adam writes through raw pointers: no derived copy of old weights)
        if self.finetune_imu:                         # (--finetune_all)
            self.model_IMU.eval()
            self.model_IMU.weights_changed()
        out, summary = evaluate_full(self, self.model_IMU, self.Upper_net, self.model, self.test_data, self.batchsize, True, self._rng,
                                     self._metrics())
        self.last_metrics = summary if self._metrics() == "full" else None
        return out


def _epoch_eval(base, dataset, batch_size, shuffle, rng, imu_net, upper_net, lower_net, metrics="reference", pose_noise=None,
                imu_noise=None, breakdown=None):
    """One evaluation pass with ONE host synchronisation: -> float64 array [n_minibatches, W] of per-frame MEANS per minibatch.
    lower_net None: W = 30, the columns of mmego_pose_errors_upper; else W = 45: the 43 columns of mmego_pose_errors, then the
    Lower stage's L1(sum) loss per frame and its mean joint distance.  The split is uploaded once per dataset object
    (DeviceArrays) and minibatches are gathered on the device in the order `data.batches` would produce (same RNG use).
    metrics="full": the same launches, and per minibatch one mmego_pose_errors_aligned launch (the 21 joints with a Lower_Net, the 15
    upper joints without) with its colsum, and -- for T >= 3 -- one mmego_pose_accel_errors launch with its colsum over the sequences,
    into further columns of the same device log: W is followed by the 3 J + 3 + len(PCK_THRESHOLDS_CM) columns of
    mmego_pose_errors_aligned (per-frame means) and J columns of acceleration error (per-sequence means; NaN when T < 3).
    pose_noise=(deg, t, seed): every minibatch's head pose is perturbed before the nets see it (ops.pose_jitter under
    pose_noise_key(seed, 0, minibatch number), rows numbered within the minibatch): what head-pose error costs in joint error.
    imu_noise=(six sigmas, seed): every minibatch's IMU samples are perturbed before IMU_Net reads them (ops.imu_jitter under
    imu_noise_key(seed, 0, minibatch number), frames and windows numbered within the minibatch): what sensor error costs.
    breakdown=(bin_cm, nbins), with a Lower_Net only: the per-minibatch tables are slices of ONE table over all rows of the pass -- the
    launches above write and read their slices, so every column keeps its bits -- and after the last minibatch evaluation.Breakdown's
    launches run over it (the grouped sums behind the log, in the same read; the histograms in one further read).  -> (the array above,
    breakdown_summary's keys).  None (the default): no launch, no allocation, the bytes of the pass without the argument."""
    if metrics not in METRICS:
        raise ValueError("metrics: %r is not one of %s" % (metrics, ", ".join(METRICS)))
    if imu_noise is not None and imu_net is None:
        raise ValueError("imu_noise perturbs what IMU_Net reads: this pass takes the head pose from the recording")
    dev = base.device
    arrays = DeviceArrays.of(dataset, dev)                  # (one copy per split, shared with eval_imu)
    todo = list(batch_indices(len(dataset), batch_size, shuffle, rng))
    W = 30 if lower_net is None else 45
    full = metrics == "full"
    J = 15 if lower_net is None else 21
    WA = ops.pose_errors_aligned_width(J, len(PCK_THRESHOLDS_CM)) if full else 0
    width = W + WA + (J if full else 0)
    bd = E_all = A_all = None
    if breakdown is not None:
        if lower_net is None:
            raise ValueError("breakdown: the figures are those of the 21 joints, so the pass needs a Lower_Net")
        win_rec, rec_action, rec_snippet = dataset_groups(dataset)
        T_all = int(np.shape(dataset._items[0])[1])
        row_rec = np.repeat(win_rec[np.concatenate(todo)] if len(todo) else win_rec[:0], T_all)          # rows in the order the pass writes them
        bd = Breakdown(breakdown, row_rec, rec_action, rec_snippet, full, dev)
        buf = torch.zeros(len(todo) * width + bd.floats(), dtype=torch.float32, device=dev)
        log = buf[:len(todo) * width].view(len(todo), width)
        E_all = torch.empty((bd.rows, 43), dtype=torch.float32, device=dev)
        A_all = torch.empty((bd.rows, WA), dtype=torch.float32, device=dev) if full else None
    else:
        log = torch.zeros((len(todo), width), dtype=torch.float32, device=dev)
    row0 = 0
    frames = np.empty(len(todo), dtype=np.float64)
    seqs = np.full(len(todo), np.nan)                       # (sequences per minibatch whose acceleration error was taken)
    scratch = base.__dict__.setdefault("_eval_scratch", {})
    lmap = scratch.get("lmap")
    if lmap is None:
        lmap = scratch["lmap"] = torch.tensor(list(base.cfg.lower_joint_map), dtype=torch.int32, device=dev)
    if full and "pck_thr" not in scratch:
        scratch["pck_thr"] = torch.tensor([c / 100.0 for c in PCK_THRESHOLDS_CM], dtype=torch.float32, device=dev)
    with torch.no_grad():
        for i, idx in enumerate(todo):
            b = arrays.gather(idx)                          # fresh copies: the nets transform `data` in place (Q1)
            B, T = b["data"].shape[0], b["data"].shape[1]
            F = B * T
            frames[i] = F
            key = (B, T, W)
            if key not in scratch:
                scratch[key] = (torch.zeros((6, B, 64), device=dev), torch.zeros((6, B, 64), device=dev),
                                torch.empty((F, 43 if lower_net is not None else 30), dtype=torch.float32, device=dev))
            h0, c0, E = scratch[key]
            if bd is not None:
                E = E_all[row0:row0 + F]
            tgt, body = b["target"], b["skl"]
            imu = b["imu"] if imu_noise is None else _jitter_imu(scratch, b["imu"], imu_noise, imu_noise_key(imu_noise[1], 0, i))
            R, t = base.head_pose(imu_net, imu, b["R_R0R"], tgt)
            if pose_noise is not None:
                R, t = _jitter_pose(scratch, R, t, pose_noise, pose_noise_key(pose_noise[2], 0, i))
            up = call_upper(upper_net, b["data"], h0, c0, body, R, t)[0]      # (an UpperNet or an UpperNetwlocal)
            lo = None
            if lower_net is None:
                hip.call("pose_errors_upper", up.contiguous(), tgt, F, E)
                ops.colsum(E, log[i])
            else:
                lo, _ = lower_net(up.clone(), b["data"], h0, h0, h0, h0, body, R, t)     # x already transformed once (Q1)
                hip.call("pose_errors", up.contiguous(), lo.contiguous(), tgt, F, E)
                ops.colsum(E, log[i, :43])
                hip.call("l1_loss", lo.contiguous(), tgt, lmap, 8, 21, F, 1.0, log[i, 43:45], None)
            if full:
                up, lo = up.contiguous().view(B, T, 15, 3), None if lo is None else lo.contiguous().view(B, T, 8, 3)
                akey = ("aligned", B, T, J)
                if akey not in scratch:
                    scratch[akey] = (torch.empty((F, WA), dtype=torch.float32, device=dev), torch.empty((B, J), dtype=torch.float32, device=dev))
                A, Acc = scratch[akey]
                if bd is not None:
                    A = A_all[row0:row0 + F]
                ops.pose_errors_aligned(up, lo, tgt, scratch["pck_thr"], A)
                ops.colsum(A, log[i, W:W + WA])
                if T >= 3:
                    ops.pose_accel_errors(up, lo, tgt, Acc)
                    ops.colsum(Acc, log[i, W + WA:])
                    seqs[i] = B
            row0 += F
        if bd is not None:
            hists = bd.launch(E_all, A_all, buf[len(todo) * width:])
    if bd is not None:
        host = buf.cpu().numpy().astype(np.float64)                          # the epoch's one device -> host read, the grouped sums behind the log
        out, groups = host[:len(todo) * width].reshape(len(todo), width), bd.summary(host[len(todo) * width:], hists.cpu().numpy())
    else:
        out = log.cpu().numpy().astype(np.float64)                           # the epoch's one device -> host read
    out[:, :W + WA] /= frames[:, None]
    out[:, W + WA:] /= seqs[:, None]
    blocks.seq_xcd_raise()          # (the frozen IMU_Net's persistent launches: invalid head poses must not become a reported metric)
    return out if bd is None else (out, groups)


def metrics_line(s):
    """One line of the --metrics full figures (the trainers' extra line per epoch)."""
    acc = "n/a" if s["accel_cm"] is None else "%.4f" % s["accel_cm"]
    return ("Aligned metrics: root-relative {:.4f} cm, rigid-aligned {:.4f} cm, PA-MPJPE {:.4f} cm, fit rotation {:.4f} deg, shift {:.4f} cm, "
            "scale {:.5f}, PCK {}, acceleration error {} cm/frame^2").format(
                s["root_rel_cm"], s["rigid_cm"], s["pa_cm"], s["align_rot_deg"], s["align_shift_cm"], s["pa_scale"],
                " ".join("@%gcm %.4f" % (c, v) for c, v in s["pck"].items()), acc)


def evaluate_full(base, imu_net, upper_net, lower_net, dataset, batch_size, shuffle, rng=None, metrics="reference", pose_noise=None,
                  imu_noise=None, breakdown=None):
    """IMU -> Upper -> Lower over a data split (reference Processor/Test/Demo_test.py:71-184, Train_Lower.py:232-332); returns
    (reference-style tuple, summary dict).  Device-resident split, one host read per pass (_epoch_eval).  metrics="full": the same
    tuple and summary keys from the same launches, and the summary also holds aligned_summary's keys for the 21 joints.
    pose_noise=(deg, t, seed), imu_noise=(six sigmas, seed): _epoch_eval's keywords.
    breakdown=(bin_cm, nbins) (evaluation.BREAKDOWN_BINS is --breakdown's), on a split that knows its recordings (a data.PosePC): the
    summary also holds evaluation.breakdown_summary's keys -- by_action and by_recording, PLAIN means over each group's frames (the
    figures above are means over minibatches of per-minibatch means; the two coincide where all minibatches have one size),
    percentiles_cm, percentile_clipped, beyond, per_joint_median_cm, pck_auc of the 21 joint errors' histogram, and breakdown itself.
    None (the default): none of these keys, the launches and bytes of the pass without the argument."""
    cfg = base.cfg
    breakdown = check_breakdown(breakdown)
    m = _epoch_eval(base, dataset, batch_size, shuffle, rng, imu_net, upper_net, lower_net, metrics, pose_noise=pose_noise,
                    imu_noise=imu_noise, breakdown=breakdown)
    groups = None
    if breakdown is not None:
        m, groups = m
    eval_loss = float(np.mean(m[:, 43]))
    accu_l, accu_up, accu_lo = m[:, :21].mean(axis=1), m[:, 41], m[:, 42]
    accu_ll, angle_ll = m[:, :21].mean(axis=0), m[:, 21:41].mean(axis=0)
    summary = dict(all_cm=float(np.mean(accu_l)) * 100, upper_cm=float(np.mean(accu_up)) * 100, lower_cm=float(np.mean(accu_lo)) * 100,
                   rot_deg=float(sum(angle_ll) / len(angle_ll)), per_joint_cm=accu_ll * 100)
    if metrics == "full":
        summary.update(aligned_summary(m[:, 45:], 21))
    if groups is not None:
        summary.update(groups)
    return (eval_loss, np.asarray([eval_loss / cfg.joint_num_lower]), float(np.mean(accu_l)), float(np.mean(accu_lo)), accu_ll, angle_ll), summary


class Evaluator(_Base):
    """`python main.py --infer` (reference Processor/Test/Demo_test.MMEgo.eval_model)."""

    def __init__(self):
        super().__init__(ConfigDemo, make_dirs=False)
        cfg = self.cfg
        self.model = LowerNet(hidden_dim=64).to(self.device).eval()
        self.model_IMU = self._load_imu()
        self.Upper_net = self._new_upper(cfg.model_upper_path).eval()           # (--upper_variant)
        # (--dense: the per-frame clouds stay; nothing else about the object depends on the keyword)
        self.vis_data = PosePC(train=False, vis=True, batch_length=self.frame_no,
                               keep_frames=bool(getattr(cfg, "dense", False) or getattr(cfg, "vis", False)))

    def eval_dense(self):
        """`--infer --dense [--stride S --blend B --smooth H --rot_smooth H --save_pred PATH --batch_size N]`: dense_infer over the recordings, its figures printed
        (the reference's five lines for the blend first), the per-frame skeletons written when asked for.  -> the summary."""
        cfg = self.cfg
        self.model.load(cfg.model_lower_path)
        self.model.eval()
        stride = cfg.stride if getattr(cfg, "stride", None) is not None else max(1, self.frame_no // 2)
        opt = dict(metrics=self._metrics(), blend_space=getattr(cfg, "blend_space", None), smooth=getattr(cfg, "smooth", None),
                   floor=getattr(cfg, "floor", None), pose_noise=pose_noise_of(cfg), imu_noise=imu_noise_of(cfg),
                   rot_smooth=getattr(cfg, "rot_smooth", None), breakdown=BREAKDOWN_BINS if getattr(cfg, "breakdown", False) else None)
        if getattr(cfg, "render", None) is not None:               # (the key only with --render: the pass without it is untouched)
            opt["render"] = cfg.render
        for key in ("online", "one_euro"):                         # (likewise)
            if getattr(cfg, key, None) is not None:
                opt[key] = getattr(cfg, key)
        s, arrays = dense_infer(self, self.model_IMU, self.Upper_net, self.model, self.vis_data, stride, blend=cfg.blend,
                                batch_size=getattr(cfg, "dense_batch_size", None) or 64, **opt)
        self.last_metrics = s
        path = getattr(cfg, "save_pred", None)
        if path:
            np.savez(path, **dense.saved_arrays(s, arrays, opt))
        dense.print_summary(s, opt, saved=path)
        return s

    def eval_model(self):
        self.model.load(self.cfg.model_lower_path)
        self.model.eval()
        noise, imu_noise = pose_noise_of(self.cfg), imu_noise_of(self.cfg)
        breakdown = BREAKDOWN_BINS if getattr(self.cfg, "breakdown", False) else None
        out, s = evaluate_full(self, self.model_IMU, self.Upper_net, self.model, self.vis_data, 1, False, metrics=self._metrics(),
                               pose_noise=noise, imu_noise=imu_noise, breakdown=breakdown)
        print_reference(s)
        if self._metrics() == "full":
            self.last_metrics = s
            print_aligned(s)
        if noise is not None:
            print(pose_noise_line(noise))
        if imu_noise is not None:
            print(imu_noise_line(imu_noise))
        if breakdown is not None:
            self.last_metrics = s
            print_breakdown(s)
        return out

    def eval_all_skeleton(self):
        """`--infer --vis` (reference Demo_test.MMEgo.eval_all_skeleton, whose drawing routine its Utils.py does not define): the dense
        pass at stride = frame_no with blend "mean" -- the reference's windows plus one head window per recording -- with every recording
        drawn on the device into ./vis/<Idx>/ at --render's defaults; prints what that dense pass prints.  -> the summary."""
        cfg = self.cfg
        self.model.load(cfg.model_lower_path)
        self.model.eval()
        opt = dict(metrics=self._metrics(), blend_space=None, smooth=None, floor=None, pose_noise=None, imu_noise=None, rot_smooth=None,
                   breakdown=None, render=(os.path.join(".", "vis", str(cfg.Idx)), RENDER_SIZE, None, RENDER_FPS))
        s, _ = dense_infer(self, self.model_IMU, self.Upper_net, self.model, self.vis_data, self.frame_no, blend="mean", batch_size=64, **opt)
        self.last_metrics = s
        dense.print_summary(s, opt)
        return s


class ImuTrainer(_Base):
    """`python main.py --train --network IMU_Net` (reference Train_IMU.MMEgo): stage 1, geodesic + 100 x position loss,
    Adam with coupled weight decay 1e-3."""
    weight_decay, net_name = 0.001, "IMU_Net"

    def __init__(self):
        super().__init__(Config)
        cfg = self.cfg
        self.num_epochs, self.save_slot, self.learning_rate = cfg.epochs, 50, cfg.lr
        self.model_IMU = IMUNet(15, 6 + 3, 512, 2, True, getattr(cfg, "imu_dropout", None) or 0).to(self.device)      # (--imu_dropout)
        if cfg.IMU_pretrained:
            self.model_IMU.load(cfg.model_IMU_path)
        self._dp_start(self.model_IMU)
        self.imu_noise = imu_noise_of(cfg)                             # (--imu_noise_*, --imu_bias_*: (six sigmas, seed) or None)
        if self.imu_noise is not None:
            self._say_imu_noise()
        self._opts = {}
        self._load_splits()
        rep = os.path.join(_TRAIN_DIR, "report", str(self.Idx))
        self.lossfile = open(os.path.join(rep, "log-loss.txt"), self._log_mode()) if self.rank == 0 else None
        self._rng = np.random.RandomState(1234)
        self._loss = torch.zeros(1, device=self.device)
        self.start_epoch, self._resume = 0, None
        self._train_dev = None
        self._steps = {}

    def train_imu_once(self):
        self.model_IMU.train()
        losses = []
        pg = self.pg
        self._train_arrays()
        for i, idx in enumerate(batch_indices(len(self.train_data), self.batchsize * self.world, True, self._rng)):
            idx = idx[shard_of(self.rank, self.world)]
            if len(idx) == 0:       # nothing for this rank in a short last global minibatch: zero gradient, same update
                empty_step(self.model_IMU, self._main_opt(self.model_IMU), pg)
                continue
            b = self._train_dev.gather(idx)
            B, T = b["imu"].shape[0], b["imu"].shape[1]
            st = self._steps.get(B)
            if st is None:                                              # one graph per minibatch size, one optimiser
                st = self._steps[B] = ImuStep(self.model_IMU, process_group=pg, use_graph=True, opt=self._main_opt(self.model_IMU),
                                              **({} if self.imu_noise is None else dict(imu_noise=self.imu_noise[0])))
                self._say_decay()
            if st.static is None or st.static["imu"].data_ptr() != b["imu"].data_ptr():
                st.bind(b["imu"], b["R_R0R"], b["target"])
            if self.imu_noise is not None:                              # this minibatch's draws (the word the captured launch reads)
                st.set_imu_key(imu_noise_key(self.imu_noise[1], self._epoch, i, self.rank))
            st.step()
            losses.append(st.loss.item() / B / T)
        return float(np.mean(losses))

    def eval_imu(self):
        """Reference Processor/Train/Train_IMU.py:151-185.  Device-resident test split, per-minibatch figures kept in a device log
        (total loss from mmego_imu_loss; the position part = sum of |t - head joint| from mmego_l1_loss's distance output), one
        host read per epoch."""
        self.model_IMU.eval()
        dev = self.device
        self._test_dev = DeviceArrays.of(self.test_data, dev)
        if getattr(self, "_head_map", None) is None:
            self._head_map = torch.tensor([20], dtype=torch.int32, device=dev)
        todo = list(batch_indices(len(self.test_data), self.batchsize, True, self._rng))
        log = torch.zeros((len(todo), 3), dtype=torch.float32, device=dev)
        frames = np.empty(len(todo), dtype=np.float64)
        with torch.no_grad():
            for i, idx in enumerate(todo):
                b = self._test_dev.gather(idx)
                B, T = b["imu"].shape[0], b["imu"].shape[1]
                F = B * T
                frames[i] = F
                head = torch.empty((B, T, 3), dtype=torch.float32, device=dev)
                ops.copy2d(b["target"].view(F, 63)[:, 60:63], head.view(F, 3))
                R, t = self.model_IMU(b["imu"])
                hip.call("imu_loss", R.contiguous(), t.contiguous(), b["R_R0R"], head, F, 1.0, log[i, 0:1], None, None)
                hip.call("l1_loss", t.contiguous(), b["target"], self._head_map, 1, 21, F, 1.0, log[i, 1:3], None)
        m = log.cpu().numpy().astype(np.float64) / frames[:, None]          # the epoch's one device -> host read
        blocks.seq_xcd_raise()
        tot, pos = m[:, 0], m[:, 2]
        return float(np.mean(tot)), np.mean(np.stack((tot - 100.0 * pos, pos), axis=1), axis=0)

    def train_imu(self):
        def report(epoch, train_loss, out):
            print("Train_loss: {}".format(train_loss))
            print("Eval_loss: {}  Eval_loss_l (angle, H_pos): {}".format(out[0], out[1]))
        self._epochs(self.model_IMU, self.train_imu_once, self.eval_imu, report)
