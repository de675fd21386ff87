#!/usr/bin/env python3
"""Command line of the reference (main.py:7-73), same flags and precedence (CLI > Config defaults):

  python main.py --train --network {IMU_Net,Upper_Net,Lower_Net} [--epochs N --lr F --batch_size N --device cuda:0
                 --log_dir IDX --load_IMU_path P --load_Upper_path P --load_Lower_path P]
  python main.py --infer [--vis | --dense [--stride S --blend {mean,triangle} --blend_space {joints,bones,rot} --save_pred PATH]]
  python main.py --infer --dense --smooth H [--smooth_order {0,1,2} --smooth_taper {box,gauss}]
  python main.py --infer --dense --blend_space rot --rot_smooth H [--rot_smooth_order {0,1,2} --rot_smooth_taper {box,gauss}]
  python main.py --infer --dense --floor {measure,clamp} [--floor_contact_cm H --floor_margin_cm M]
  python main.py --infer --dense --online [--lookahead L] [--one_euro FC [--one_euro_beta B --one_euro_dcutoff DC]]
  python main.py --infer [--dense ...] --breakdown
  python main.py --infer --dense --render DIR [--render_size PX --render_recordings 0,3,7 --render_fps N]

Added flags (not in the reference): --gt_head_pose (use the recorded head pose when no IMU_Net checkpoint is
available), --data_root, --seed, --resume (bit-exact continuation: weights, Adam moments/step, epoch, RNG states),
--finetune_imu [--imu_lr F] (stage 2 trains the IMU_Net too, through Upper_Net's head-pose gradients), --finetune_upper [--upper_lr F]
(stage 3 trains the Upper_Net too, through Lower_Net's input gradients, on the sum of the two stages' losses), --finetune_all [--upper_lr F
--imu_lr F] (stage 3 trains all three nets end to end on that sum: IMU_Net through Upper_Net's and Lower_Net's head-pose gradients),
--imu_dropout P (the IMU_Net that is TRAINED -- stage 1, --finetune_imu or --finetune_all -- gets nn.LSTM(dropout=P) between its BiLSTM layers), --clip_grad_norm X (every
trained net's gradient is clipped to the global norm X ahead of its Adam step; steps with a non-finite gradient are skipped; one
"Grad norm" line per net and epoch; `inf` only measures), --ema_decay D (every trained net keeps an exponential moving average of its
weights at decay D, updated inside its fused Adam launch; each epoch's evaluation, model selection and early stopping run on the averaged
weights; the checkpoints keep the raw weights and the averaged nets are written beside them under EMA/), --lr_schedule {cosine,linear,step}
[--lr_warmup N --lr_min_ratio R --lr_decay_steps N --lr_step_every N --lr_step_gamma G] (every trained net's learning rate follows a warm-up
and a decay over its optimiser's step count, computed inside its fused Adam launch; --lr_warmup alone: warm-up, then constant),
--weight_decay W [--decay_mode {l2,adamw} --no_decay_1d] (the weight decay of every trained net in place of the reference's, coupled or
decoupled at the rate of the step, optionally leaving biases and normalisation parameters out, inside its fused Adam launch), --upper_variant {global,wlocal} (which net "Upper_Net" is: UpperNet, or
UpperNetwlocal with the anchor branch -- the net trained by --train --network Upper_Net, the class the Upper checkpoint is loaded into by
--train --network Lower_Net and --infer), --metrics {reference,full} (full: beside the reference's figures, the evaluation pass of --infer
and of --train --network Upper_Net / Lower_Net also takes root-relative, rigid-aligned and Procrustes-aligned joint errors, the fit's
rotation, shift and scale, PCK and the acceleration error on the device -- pose error apart from placement error; printed only, the log
files keep their format), --window_jitter (every epoch each training window moves to a valid start within +-(frame_no-1) frames of its
own), --point_keep P (every minibatch's clouds are packed afresh on the device, each radar return kept with probability P) and
--point_noise S / --point_noise_v S (that device packing also jitters every kept return: x, y, z by a bell-shaped draw of standard deviation
S metres, clipped at +-3.46 S, with r recomputed from the result, and the Doppler velocity likewise in its own units): what a
run is trained on, from the frame-major device store data.FrameStore; evaluation is untouched; --infer --dense [--stride S --blend
{mean,triangle} --blend_space {joints,bones,rot} --save_pred PATH] (sliding-window inference over whole recordings: the three nets run over overlapping windows S frames
apart, every frame's pose is blended on the device from the windows that cover it, the blended and the single-window errors, the error
by position in the window and the windows' disagreement are printed, and PATH receives the per-frame skeletons; --blend_space bones
blends bone directions and keeps the body's bone lengths, so that a blended frame is a rigid skeleton again; --blend_space rot averages
the world rotations both nets predicted for every bone over the windows and runs the nets' forward kinematics once on the averages --
rigid frames too, with the twist about every bone kept -- prints the windows' rotational disagreement in degrees and adds a unit
quaternion per bone and frame (rot), rot_spread and the rest bones (bone_vectors) to PATH; it does not go with --smooth but has a filter
of its own, --rot_smooth H [--rot_smooth_order D --rot_smooth_taper {box,gauss}]: every bone's world rotation is filtered along time on the
device -- the proper rotation nearest the local polynomial of degree D of the rotations over +-H frames, the chordal mean at D = 0 -- and the
skeleton is laid along the filtered rotations, so the saved rot still produces pred; the blended frames' figures, the displacement, the
mean turn and the rotational jitter before and after the filter are printed; --smooth H [--smooth_order D
--smooth_taper {box,gauss}] then filters every recording's stitched frames along time on the device, a zero-phase local polynomial of
degree D over +-H frames -- of bone directions under --blend_space bones -- and prints the blended frames' figures and the mean
displacement beside the smoothed ones'; --floor {measure,clamp} [--floor_contact_cm H --floor_margin_cm M] reads every frame's recorded
floor plane and foot-contact flags, prints how often and how deep the saved feet lie under the floor, how well "foot lower than H cm"
reproduces the recorded contacts and how far the flagged feet hover, each beside the recorded skeleton's own figure, and under clamp
first raises every leg whose foot or ankle lies under M cm on the device, a two-bone solve that keeps the frame's bone lengths; it comes
behind the blend and the filter, and clamp does not go with --blend_space rot), --pose_noise_deg D /
--pose_noise_t S (the head pose Upper_Net and Lower_Net get -- the recording's under --gt_head_pose, else the frozen IMU_Net's -- is
perturbed per frame on the device: a random rotation whose rotation vector has standard deviation D degrees per axis, never beyond 6 D in
all, and a random shift of standard deviation S metres per component, never beyond 3.47 S.  With --train --network Upper_Net / Lower_Net
the draw is renewed every minibatch inside the captured step, as a function of (--seed, epoch, minibatch, rank), and the epoch evaluation
is untouched; with --infer and --infer --dense it is a sensitivity instrument -- how much joint error a degree or a centimetre of
head-pose error costs -- and one "Head Pose Noise" line follows the figures), --imu_noise_rot_deg D / --imu_noise_acc S / --imu_noise_gyro S
and --imu_bias_rot_deg D / --imu_bias_acc S / --imu_bias_gyro S (the 20 x 15 IMU samples per frame that IMU_Net reads are perturbed on the
device: white noise drawn per sample, and a bias that stays constant over a window, each on the orientation -- a rotation, degrees per axis
-- the accelerometer and the gyroscope; with --train, for every --network and with --finetune_imu / --finetune_all, re-drawn every
minibatch inside the captured step; with --infer [--dense] a sensitivity instrument, one "IMU Noise" line following the figures),
--breakdown (with --infer, with or without --dense and with every dense option: the joint error by action -- the number an action's
directory is named by -- and by recording as plain means over each group's frames, reduced on the device by a group id per frame, and
the distribution of the 21 joint errors from a device histogram of 0.05 cm bins: p50 / p90 / p95 / p99, the PCK area under 15 cm, every
joint's median, the five worst recordings; printed behind every other line, and --save_pred's file gains action, by_action_*,
by_recording_all_cm, error_hist and error_hist_bin_cm), --infer --dense --render DIR [--render_size PX --render_recordings LIST
--render_fps N] (the dense pass's FINAL frames -- behind blend, filter and clamp -- drawn on the device, one animated PNG per recording in
DIR: predicted skeleton coloured by error over the recorded one, the radar returns coloured by Doppler, the floor ring and the skeleton's
shadow on the recorded plane, front view left and side view right in a body-fixed camera; --infer --vis is that pass at the reference's
windows, drawn into ./vis/<Idx>/), --infer --dense --online [--lookahead L] (what a running device could have answered L frames after
the frame: every frame is blended from the windows that had ended by then alone, the first frame_no - 1 - L frames of a recording are
the warm-up and count as uncovered, --stride defaults to min(L + 1, frame_no // 2); not with --smooth / --rot_smooth, which read ahead)
and --infer --dense --one_euro FC [--one_euro_beta B --one_euro_dcutoff DC] (the one-euro filter along time on the device, where
--smooth sits: a causal low-pass per joint of minimum cutoff FC cycles per frame, raised by B per metre per frame of the joint's own
speed, the speed estimate's cutoff DC; of bone vectors under --blend_space bones; with or without --online, not with --smooth,
--rot_smooth or --blend_space rot).  Under `python -m torch.distributed.run --nproc-per-node N main.py --train ...` training is
data parallel (one rank per GPU, RCCL gradient all-reduce).
"""
import argparse
import os
import re

import torch

from mmego_amd.config import IMU_NOISE_FLAGS, RENDER_FPS, RENDER_SIZE, Config, ConfigDemo


def build_parser():
    p = argparse.ArgumentParser(description="Processor collection")
    p.add_argument("--network", type=str, choices=["IMU_Net", "Upper_Net", "Lower_Net"],
                   help="Choose a network: IMU_Net, Upper_Net, Lower_Net")
    p.add_argument("--train", action="store_true", help="Train model")
    p.add_argument("--infer", action="store_true", help="Perform inference")
    p.add_argument("--vis", action="store_true", help="Visualization")
    p.add_argument("--colab", action="store_true", help="Called by colab")
    p.add_argument("--epochs", type=int, help="Number of epochs")
    p.add_argument("--lr", type=float, help="Learning rate")
    p.add_argument("--device", type=str, help="device: [cuda:no, cpu]")
    p.add_argument("--batch_size", type=int, help="Batch size")
    p.add_argument("--log_dir", type=int, help="Path to save the model and report")
    p.add_argument("--load_IMU_path", type=str, help="Path to load IMU_Net")
    p.add_argument("--load_Upper_path", type=str, help="Path to load Upper_Net")
    p.add_argument("--load_Lower_path", type=str, help="Path to load Lower_Net")
    p.add_argument("--gt_head_pose", action="store_true", help="head pose from the recording instead of IMU_Net")
    p.add_argument("--data_root", type=str, help="Sample_data directory")
    p.add_argument("--seed", type=int, help="seed torch (net initialisation) and numpy (point-cloud padding) -- the reference does not seed")
    p.add_argument("--imu_precision", type=str, choices=["fp32", "split3", "bf16"],
                   help="eval-mode IMU_Net forwards (stages 2/3, --infer): fp32 (default), split3 (fp32-accurate piece products on the "
                        "bf16 matrix pipe, inside the parity bars: DESIGN.md 7c) or bf16 product operands with fp32 accumulation "
                        "(DESIGN.md 7a, outside them)")
    p.add_argument("--imu_train_precision", type=str, choices=["fp32", "split3"],
                   help="stage-1 IMU_Net training: fp32 (default) or split3 (rnn_fast's projection / input-gradient / weight-gradient "
                        "products as piece products: DESIGN.md 7c)")
    p.add_argument("--resume", type=str, help="continue --train from a checkpoint written by this framework (the model .pth "
                                               "or its .train_state.pth: weights, Adam state, epoch, RNGs)")
    p.add_argument("--finetune_imu", action="store_true",
                   help="--train --network Upper_Net only: train the IMU_Net as well, end to end through the pose loss (Train_Upper.py:162 "
                        "without its .detach()); the IMU_Net is saved beside the Upper_Net checkpoint, in an IMU_Net folder")
    p.add_argument("--imu_lr", type=float, help="learning rate of the IMU_Net under --finetune_imu (default: --lr / Config.lr)")
    p.add_argument("--imu_dropout", type=float,
                   help="--train --network IMU_Net, or --finetune_imu: inter-layer LSTM dropout rate in [0, 1) of the IMU_Net that is "
                        "trained (default: none, as the reference's stage 1)")
    p.add_argument("--finetune_upper", action="store_true",
                   help="--train --network Lower_Net only: train the Upper_Net as well (Train_Lower.py:195-196 without its .detach()), on "
                        "the sum of the two stages' losses; the Upper_Net is saved beside the Lower_Net checkpoint, in an Upper_Net folder")
    p.add_argument("--upper_lr", type=float, help="learning rate of the Upper_Net under --finetune_upper (default: --lr / Config.lr)")
    p.add_argument("--finetune_all", action="store_true",
                   help="--train --network Lower_Net only: train IMU_Net, Upper_Net and Lower_Net together on loss_lower + loss_upper "
                        "(IMU_Net through both nets' head-pose gradients; it means --finetune_imu and --finetune_upper for stage 3 and is "
                        "given without them); the two nets are saved beside the Lower_Net checkpoint, in IMU_Net and Upper_Net folders; "
                        "--upper_lr, --imu_lr and --imu_dropout apply")
    p.add_argument("--clip_grad_norm", type=float,
                   help="--train: clip every trained net's gradient to this global norm ahead of its Adam step (one clip_grad_norm_ per "
                        "optimiser, on the SUM-loss gradient of the global minibatch), skip a step whose gradient is not finite, and print "
                        "the norms once per epoch; `inf` measures without clipping (default: no clipping)")
    p.add_argument("--ema_decay", type=float,
                   help="--train: every trained net keeps an exponential moving average of its weights, ema += (1 - D)(w - ema) after each "
                        "Adam step, D in (0, 1), starting from the weights the run starts from; each epoch's evaluation pass, model "
                        "selection and early stopping use the averaged weights.  Checkpoints keep the raw weights (the average travels in "
                        "the optimiser state, so --resume continues it without the flag); the averaged nets are written in the "
                        "reference's format beside them, in an EMA folder (default: no averaging)")
    p.add_argument("--lr_schedule", type=str, choices=["cosine", "linear", "step"], default=None,
                   help="--train: every trained net's learning rate follows this schedule over its optimiser's step count, computed inside "
                        "the fused Adam launch (skipped steps consume none): cosine / linear decay to --lr_min_ratio x lr over "
                        "--lr_decay_steps steps (default: the rest of the run), or step (x --lr_step_gamma every --lr_step_every steps, "
                        "not below --lr_min_ratio).  --resume continues the saved schedule without the flags (default: constant)")
    p.add_argument("--lr_warmup", type=int, help="--train: linear warm-up over the first N >= 1 optimiser steps (step 1 at lr / N, step N "
                                                  "the first at the full rate), ahead of --lr_schedule's decay or, alone, of a constant rate")
    p.add_argument("--lr_min_ratio", type=float, help="--lr_schedule: where the decay ends, as a fraction of lr, in [0, 1) (default 0)")
    p.add_argument("--lr_decay_steps", type=int, help="--lr_schedule cosine / linear: the N >= 1 optimiser steps the decay takes behind "
                                                       "the warm-up (default: epochs x minibatches per epoch - warm-up)")
    p.add_argument("--lr_step_every", type=int, help="--lr_schedule step: decay every N >= 1 optimiser steps behind the warm-up")
    p.add_argument("--lr_step_gamma", type=float, help="--lr_schedule step: the factor of each decay, in (0, 1]")
    p.add_argument("--weight_decay", type=float,
                   help="--train: the weight decay W >= 0 of every net the run trains, in place of the reference's (IMU_Net 1e-3, Upper_Net "
                        "and Lower_Net 0), applied inside the fused Adam launch.  --resume continues the saved setting without the flags")
    p.add_argument("--decay_mode", type=str, choices=["l2", "adamw"], default=None,
                   help="--weight_decay: l2 (default: W x weight joins the gradient, as torch.optim.Adam does) or adamw (decoupled: the "
                        "weight shrinks by lr_t x W ahead of the update, lr_t the rate of the step, the scheduled one under --lr_schedule)")
    p.add_argument("--no_decay_1d", action="store_true",
                   help="--weight_decay: parameters with at most one dimension (biases, BatchNorm scales and shifts, LSTM biases) do not decay")
    p.add_argument("--upper_variant", type=str, choices=["global", "wlocal"], default=None,
                   help="which net Upper_Net is: global (default: UpperNet) or wlocal (UpperNetwlocal, with the anchor branch).  --train "
                        "--network Upper_Net trains it (with --finetune_imu, --imu_lr, --imu_dropout, --clip_grad_norm, --resume and "
                        "--gt_head_pose as for global); --train --network Lower_Net and --infer load the Upper checkpoint into it.  wlocal "
                        "stays frozen in stage 3: not with --finetune_upper / --finetune_all")
    p.add_argument("--metrics", type=str, choices=["reference", "full"], default="reference",
                   help="figures of the evaluation pass: reference (default: what the reference reports) or full (also root-relative, "
                        "rigid-aligned and Procrustes-aligned joint errors, the alignment's rotation / shift / scale, PCK at 5, 10 and 15 cm "
                        "and the acceleration error, computed on the device in the same pass).  --infer prints them behind the "
                        "reference's lines; --train --network Upper_Net / Lower_Net prints one more line per epoch (stdout only; model "
                        "selection and early stopping do not look at them)")
    p.add_argument("--window_jitter", action="store_true",
                   help="--train: every epoch moves each training window to a start drawn uniformly from the valid starts within "
                        "+-(frame_no - 1) frames of its own (one recording, no frame of a test window; frames outside the reference's "
                        "window grid are used).  Draws are functions of (--seed, epoch); evaluation stays on the reference's test windows")
    p.add_argument("--point_keep", type=float,
                   help="--train --network Upper_Net / Lower_Net: every minibatch's point clouds are packed afresh on the device from the "
                        "raw radar returns, each return kept with probability P in (0, 1] (1: only the packing is re-drawn); draws are "
                        "functions of (--seed, epoch, minibatch).  Evaluation stays on the loader's packing")
    p.add_argument("--point_noise", type=float,
                   help="--train --network Upper_Net / Lower_Net: metres, the standard deviation of the jitter on x, y and z of every radar "
                        "return, added on the device while every minibatch's clouds are packed afresh (without --point_keep every return "
                        "is kept and only the packing is re-drawn); a centred sum of four uniforms, so no draw lies beyond +-3.46 S; r is "
                        "recomputed from the result.  Draws are functions of (--seed, epoch, minibatch).  Evaluation stays on the "
                        "loader's packing")
    p.add_argument("--point_noise_v", type=float,
                   help="--train --network Upper_Net / Lower_Net: the same on the Doppler velocity of every radar return, in the "
                        "recordings' units")
    p.add_argument("--pose_noise_deg", type=float,
                   help="--train --network Upper_Net / Lower_Net, or --infer [--dense]: degrees, the standard deviation PER AXIS of a random "
                        "rotation vector applied to every frame's head pose before the nets see it (RMS rotation angle sqrt(3) D, never "
                        "beyond 6 D; a centred sum of four uniforms per axis).  Training: re-drawn every minibatch on the device from "
                        "(--seed, epoch, minibatch, rank), so --resume continues the sequence; the epoch evaluation is untouched.  --infer: "
                        "drawn from --seed; --dense gives a frame one pose error in every window that serves it.  Not with "
                        "--finetune_imu / --finetune_all (no gradient flows through the perturbation)")
    p.add_argument("--pose_noise_t", type=float,
                   help="the same on the head position: metres, the standard deviation per component of a random shift (never beyond "
                        "3.47 S).  Either flag may be given without the other")
    p.add_argument("--imu_noise_rot_deg", type=float,
                   help="--train (any --network that runs an IMU_Net, --finetune_imu / --finetune_all included) or --infer [--dense]: white "
                        "noise on the ORIENTATION of every IMU sample IMU_Net reads -- degrees, the standard deviation PER AXIS of a random "
                        "rotation vector, drawn anew for each of a frame's 20 samples (never beyond 6 D).  Training: re-drawn every minibatch "
                        "on the device from (--seed, epoch, minibatch, rank), so --resume continues the sequence; the epoch evaluation is "
                        "untouched.  --infer: drawn from --seed; --dense keeps a frame's white noise in every window that serves it.  Any "
                        "subset of the six --imu_noise_* / --imu_bias_* flags may be given; not with --gt_head_pose (no IMU_Net runs) "
                        "unless --train --network IMU_Net")
    p.add_argument("--imu_noise_acc", type=float,
                   help="the same on the accelerometer: the standard deviation per component of an added draw, in the recordings' units "
                        "(never beyond 3.47 S)")
    p.add_argument("--imu_noise_gyro", type=float, help="the same on the gyroscope")
    p.add_argument("--imu_bias_rot_deg", type=float,
                   help="a BIAS on the orientation: one random rotation per window (degrees per axis of its rotation vector), the same for "
                        "all frame_no x 20 samples of the window, applied together with --imu_noise_rot_deg's; under --infer --dense a bias "
                        "belongs to its window")
    p.add_argument("--imu_bias_acc", type=float, help="a bias on the accelerometer: one offset per window and component, in the recordings' units")
    p.add_argument("--imu_bias_gyro", type=float, help="the same on the gyroscope")
    p.add_argument("--dense", action="store_true",
                   help="--infer only: sliding-window inference over whole recordings -- overlapping frame_no-frame windows --stride frames "
                        "apart (tail-anchored, plus one window at every recording's head), every frame's pose blended on the device from "
                        "the windows that cover it.  Prints the reference's five lines for the blend, the single-window figures, the error "
                        "by position in the window, the windows' mean disagreement and the plan's counts (--metrics full: the aligned lines, "
                        "the acceleration error per recording, across window seams); --batch_size is the window minibatch (default 64)")
    p.add_argument("--stride", type=int, help="--dense: frames between window starts, in [1, frame_no] (default: frame_no // 2)")
    p.add_argument("--blend", type=str, choices=["mean", "triangle"], default=None,
                   help="--dense: weight of a window's prediction for a frame -- mean (default: 1) or triangle (min(p + 1, frame_no - p) at "
                        "position p: the window's middle counts most)")
    p.add_argument("--blend_space", type=str, choices=["joints", "bones", "rot"], default=None,
                   help="--dense: what is blended over a frame's windows -- joints (default: every joint's 3-vector on its own; where the "
                        "windows disagree about a bone's direction the blended bone comes out shorter) or bones (every bone's direction, set "
                        "to the body's bone length and laid along the kinematic tree from the blended roots: the frames stay rigid "
                        "skeletons) or rot (every bone's world rotation as the nets predicted it, averaged over the windows -- the weighted "
                        "chordal mean -- and the nets' forward kinematics run once on the averages: rigid frames with the twist about every "
                        "bone kept; one more line gives the windows' rotational disagreement in degrees, and --save_pred's file gains rot "
                        "[F, 20, 4], a unit quaternion (w, x, y, z) per bone and frame in the world frame, rot_spread [F] and bone_vectors "
                        "[20, 3], the rest bones: rot applied to bone_vectors from pred's roots gives pred.  Not with --smooth; --rot_smooth "
                        "filters the rotations along time).  Given, any "
                        "value prints one more line, the blended and single-window deviation from the bone "
                        "lengths, and adds blend_space and degenerate_bones to --save_pred's file")
    p.add_argument("--save_pred", type=str,
                   help="--dense: write the per-frame arrays to this .npz -- pred [F, 21, 3] (NaN where no window covers the frame: "
                        "recordings shorter than frame_no), covered, spread, recording, frame_in_recording, target, stride, blend, frame_no")
    p.add_argument("--smooth", type=int, metavar="H",
                   help="--dense: smooth every recording's stitched poses along time on the device, after the blend -- a zero-phase "
                        "local-polynomial filter over the frames f-H .. f+H of the same recording, H in [1, 31] (off by default).  Under "
                        "--blend_space bones the bone directions are filtered and the frames stay rigid.  The figures above are then the "
                        "smoothed frames'; three more lines give the blended frames' error, the mean displacement and (--metrics full) the "
                        "unsmoothed acceleration error, and --save_pred's file gains pred_unsmoothed, moved, smooth_window, smooth_order, "
                        "smooth_taper")
    p.add_argument("--smooth_order", type=int, choices=[0, 1, 2], default=None,
                   help="--smooth: degree of the local polynomial (default 2; 0 is a weighted moving average)")
    p.add_argument("--smooth_taper", type=str, choices=["box", "gauss"], default=None,
                   help="--smooth: weights of the frames of the window -- box (ones) or gauss (default: exp(-2 k^2 / H^2), sigma H / 2)")
    p.add_argument("--rot_smooth", type=int, metavar="H",
                   help="--dense --blend_space rot: filter every bone's blended world rotation along time on the device -- with --smooth's "
                        "taps and weights over the frames f-H .. f+H of the same recording, H in [1, 31], the proper rotation nearest the "
                        "local polynomial of the rotation matrices (order 0: the weighted chordal mean of the neighbouring frames) -- and "
                        "lay the rest bones along the filtered rotations from the filtered roots: rigid frames whose saved rot still "
                        "produces pred (off by default).  The figures above are then the filtered frames'; more lines give the blended "
                        "frames' error, the displacement with the mean turn, the rotational jitter before and after the filter and "
                        "(--metrics full) the unsmoothed acceleration error, and --save_pred's file gains pred_unsmoothed, rot_unsmoothed, "
                        "moved, rot_moved, rot_smooth_window, rot_smooth_order, rot_smooth_taper")
    p.add_argument("--rot_smooth_order", type=int, choices=[0, 1, 2], default=None,
                   help="--rot_smooth: degree of the local polynomial (default 2; 0 is the weighted chordal mean)")
    p.add_argument("--rot_smooth_taper", type=str, choices=["box", "gauss"], default=None,
                   help="--rot_smooth: weights of the frames of the window -- box or gauss (default), as --smooth_taper")
    p.add_argument("--online", action="store_true",
                   help="--dense: what a running device could have answered -- frame f is blended from the windows that had ended by "
                        "f + --lookahead alone.  The first frame_no - 1 - L frames of every recording are the warm-up (no full window yet) "
                        "and count as uncovered; --stride defaults to min(L + 1, frame_no // 2) and may not exceed L + 1.  Not with "
                        "--smooth or --rot_smooth (they read H frames ahead); --one_euro is the causal filter.  One 'Online' line in "
                        "front of the counts; --save_pred's file gains online_lookahead")
    p.add_argument("--lookahead", type=int, default=None, metavar="L",
                   help="--online: the latency budget in frames, in [0, frame_no - 1] (default 0: a frame is answered by the one window "
                        "that ends at it)")
    p.add_argument("--one_euro", type=float, default=None, metavar="FC",
                   help="--dense: the one-euro filter (Casiez et al. 2012) along time on the device, after the blend where --smooth sits "
                        "-- a causal exponential low-pass per joint whose cutoff is FC + B |speed| cycles per frame, so it never reads a "
                        "frame ahead; FC finite and > 0.  Under --blend_space bones every bone's vector is filtered and the body's bone "
                        "lengths are kept.  Three more lines give the blended frames' error, the mean displacement and (--metrics full) "
                        "the unsmoothed acceleration error; --save_pred's file gains pred_unsmoothed, moved, one_euro_cutoff, "
                        "one_euro_beta, one_euro_dcutoff.  Not with --smooth, --rot_smooth or --blend_space rot")
    p.add_argument("--one_euro_beta", type=float, default=None, metavar="B",
                   help="--one_euro: how much a joint's speed in metres per frame raises the cutoff, in 1/metre, finite and >= 0 "
                        "(default 0: a plain exponential filter)")
    p.add_argument("--one_euro_dcutoff", type=float, default=None, metavar="DC",
                   help="--one_euro: cutoff of the speed estimate in cycles per frame, finite and > 0 (default 0.1: the filter's usual "
                        "1 Hz at the recordings' 10 frames per second)")
    p.add_argument("--floor", type=str, choices=["measure", "clamp"], default=None,
                   help="--dense: hold the saved feet against every frame's recorded floor plane (given in the frame of the frame's own "
                        "joints; it comes from the recording, as the head pose does under --gt_head_pose) and the recorded foot-contact "
                        "flags, behind the blend and --smooth.  measure prints the foot height error, the floor penetration rate and "
                        "depth, precision and recall of 'foot lower than --floor_contact_cm' against the flags and the hover of the "
                        "flagged feet, with the recorded skeleton's own figures beside them; clamp first raises every leg whose foot or "
                        "ankle lies under --floor_margin_cm (a two-bone solve on the device that keeps the frame's bone lengths), reports "
                        "the clamped frames and keeps the unclamped figures beside them (not with --blend_space rot).  --save_pred's file "
                        "gains foot_height, ground, foot_contact, floor_mode, floor_contact_cm, floor_margin_cm, and under clamp "
                        "pred_unclamped, lifted, floor_fallback")
    p.add_argument("--floor_contact_cm", type=float, default=None, metavar="H",
                   help="--floor: a foot lower than H cm above the floor counts as in contact (default 6, between the flagged and the "
                        "unflagged feet of the 21 frames the test fixture stores; no claim for the full data)")
    p.add_argument("--floor_margin_cm", type=float, default=None, metavar="M",
                   help="--floor clamp: feet and ankles are raised to M cm above the floor (default 0)")
    p.add_argument("--breakdown", action="store_true",
                   help="--infer [--dense]: break the error down on the device -- one line per action (the number its directory is named "
                        "by) with the mean joint, upper, lower and rotation error over the action's frames, its p50 and p90 (--metrics "
                        "full: PA-MPJPE and root-relative error too), the five worst recordings, and the distribution of all joint errors "
                        "from a histogram of 0.05 cm bins up to 204.75 cm: p50, p90, p95, p99, the PCK area under 15 cm and every joint's "
                        "median.  Group figures are plain means over frames.  Printed behind every other line; --dense takes them on the "
                        "final frames and --save_pred's file gains action, by_action_*, by_recording_all_cm, error_hist, error_hist_bin_cm")
    p.add_argument("--render", type=str, metavar="DIR",
                   help="--dense: draw the final frames of every recording that has a covered frame on the device and write one "
                        "animated PNG per recording into DIR, rec{recording:04d}_action{A}.png: the prediction coloured by its error "
                        "over the recorded skeleton, the radar returns coloured by Doppler velocity, a 1 m ring and the prediction's "
                        "shadow on the recorded floor plane; front view left, side view right, in a camera fixed to the recorded body "
                        "(off by default; not with --vis, which draws into ./vis/<Idx>/ on its own)")
    p.add_argument("--render_size", type=int, default=None, metavar="PX",
                   help="--render: a view is PX x PX pixels and a frame PX x 2 PX; a multiple of 4 in [64, 1024] (default 256)")
    p.add_argument("--render_recordings", type=str, default=None, metavar="LIST",
                   help="--render: comma-separated loader recording numbers, as --save_pred's `recording` counts them (default: all)")
    p.add_argument("--render_fps", type=int, default=None, metavar="N", help="--render: frames per second of the animation, in [1, 100] (default 10)")
    return p


def parse_recordings(text):
    """--render_recordings' value "0,3,7" -> [0, 3, 7]; None where it is no comma-separated list of integers >= 0."""
    if not re.fullmatch(r"[0-9]+(,[0-9]+)*", text):
        return None
    return [int(p) for p in text.split(",")]


def check_render(parser, args):
    """--render is a stage of --infer --dense; --render_size, --render_recordings and --render_fps belong to it."""
    given = [flag for flag in ("render", "render_size", "render_recordings", "render_fps") if getattr(args, flag) is not None]
    if not given:
        return
    if args.render is not None and args.vis:
        parser.error("--render does not go with --vis: --vis draws every recording into ./vis/<Idx>/ on its own")
    if not args.dense:
        parser.error("--%s belongs to --infer --dense (sliding-window inference); without --dense nothing reads it" % given[0])
    if args.render is None:
        parser.error("--%s belongs to --render DIR: without --render nothing is drawn" % given[0])
    if args.render_size is not None and not (64 <= args.render_size <= 1024 and args.render_size % 4 == 0):
        parser.error("--render_size is a view's edge in pixels: a multiple of 4 in [64, 1024], got %d" % args.render_size)
    if args.render_recordings is not None and parse_recordings(args.render_recordings) is None:
        parser.error("--render_recordings is a comma-separated list of loader recording numbers >= 0 (0,3,7), got %r" % args.render_recordings)
    if args.render_fps is not None and not 1 <= args.render_fps <= 100:
        parser.error("--render_fps is the animation's frames per second: it has to lie in [1, 100], got %d" % args.render_fps)


def check_breakdown(parser, args):
    """--breakdown adds figures to an inference pass that compares skeletons: --infer, with or without --dense."""
    if not args.breakdown:
        return
    if args.train:
        parser.error("--breakdown does not go with --train: it breaks down an inference pass (the epochs' evaluation prints no breakdown)")
    if not args.infer:
        parser.error("--breakdown goes with --infer only (with or without --dense): it adds figures to that pass")
    if args.vis:
        parser.error("--breakdown does not go with --vis")
    if args.network == "IMU_Net":
        parser.error("--breakdown does not go with --network IMU_Net: stage 1 evaluates a head pose, there is no joint error to break down")


def check_online(parser, args):
    """--online [--lookahead L] and --one_euro FC [--one_euro_beta B --one_euro_dcutoff DC] are stages of --infer --dense."""
    given = (["online"] if args.online else []) + [f for f in ("lookahead", "one_euro", "one_euro_beta", "one_euro_dcutoff")
                                                     if getattr(args, f) is not None]
    if given and not (args.dense and args.infer):
        parser.error("--%s belongs to --infer --dense (sliding-window inference); without --dense nothing reads it" % given[0])
    if args.lookahead is not None and not args.online:
        parser.error("--lookahead belongs to --online: without --online every frame is blended from all its windows")
    if args.lookahead is not None and not 0 <= args.lookahead <= Config.frame_no - 1:
        parser.error("--lookahead is the latency budget in frames: it has to lie in [0, %d] (frame_no - 1; %d is the offline cover), got %d"
                     % (Config.frame_no - 1, Config.frame_no - 1, args.lookahead))
    for flag in ("one_euro_beta", "one_euro_dcutoff"):
        if getattr(args, flag) is not None and args.one_euro is None:
            parser.error("--%s belongs to --one_euro FC: without --one_euro nothing is filtered" % flag)
    finite = lambda v: v == v and abs(v) != float("inf")
    if args.one_euro is not None and not (finite(args.one_euro) and args.one_euro > 0.0):
        parser.error("--one_euro is the filter's minimum cutoff in cycles per frame: finite and > 0, got %r" % args.one_euro)
    if args.one_euro_beta is not None and not (finite(args.one_euro_beta) and args.one_euro_beta >= 0.0):
        parser.error("--one_euro_beta is the speed coefficient in 1/metre: finite and >= 0, got %r" % args.one_euro_beta)
    if args.one_euro_dcutoff is not None and not (finite(args.one_euro_dcutoff) and args.one_euro_dcutoff > 0.0):
        parser.error("--one_euro_dcutoff is the speed estimate's cutoff in cycles per frame: finite and > 0, got %r" % args.one_euro_dcutoff)
    for other in ("smooth", "rot_smooth"):
        if args.online and getattr(args, other) is not None:
            parser.error("--online does not go with --%s: that filter reads H frames ahead of the frame it writes, which is what --online "
                         "promises not to do (--one_euro FC filters along time without looking ahead)" % other)
        if args.one_euro is not None and getattr(args, other) is not None:
            parser.error("--one_euro does not go with --%s: it sits where that filter sits, and one pass runs one filter along time" % other)
    if args.one_euro is not None and args.blend_space == "rot":
        parser.error("--one_euro does not go with --blend_space rot: the filter runs on joint positions, so the saved rotations would "
                     "not be filtered with the positions (a causal filter of rotations is not provided)")
    if args.online and args.stride is not None and args.stride > (args.lookahead or 0) + 1:
        parser.error("--stride has to lie in [1, %d] under --online --lookahead %d: frame f is served by the windows that ended by f + %d, "
                     "so a larger stride leaves frames between windows uncovered, got %d"
                     % ((args.lookahead or 0) + 1, args.lookahead or 0, args.lookahead or 0, args.stride))


def check_dense(parser, args):
    """--dense is a mode of --infer; --stride, --blend, --blend_space, --save_pred, the --smooth, --rot_smooth and --floor flags belong to it."""
    for flag in ("rot_smooth_order", "rot_smooth_taper"):
        if getattr(args, flag) is not None and args.rot_smooth is None and args.dense:
            parser.error("--%s belongs to --rot_smooth H: without --rot_smooth no rotation is filtered" % flag)
    if args.rot_smooth is not None and not 1 <= args.rot_smooth <= 31:
        parser.error("--rot_smooth is the filter's half-width in frames: it has to lie in [1, 31] (2 H + 1 taps fit one wave), got %d"
                     % args.rot_smooth)
    if args.dense and args.rot_smooth is not None and args.blend_space != "rot":
        parser.error("--rot_smooth belongs to --dense --blend_space rot: it filters the blended rotations, which only that space keeps "
                     "(--smooth filters the positions of the other spaces)")
    for flag in ("smooth_order", "smooth_taper"):
        if getattr(args, flag) is not None and args.smooth is None and args.dense:
            parser.error("--%s belongs to --smooth H: without --smooth nothing is filtered" % flag)
    for flag in ("floor_contact_cm", "floor_margin_cm"):
        if getattr(args, flag) is not None and args.floor is None and args.dense:
            parser.error("--%s belongs to --floor {measure,clamp}: without --floor nothing reads the floor" % flag)
    if args.floor_contact_cm is not None and not 0.0 < args.floor_contact_cm < float("inf"):
        parser.error("--floor_contact_cm is a height in centimetres, finite and > 0, got %r" % args.floor_contact_cm)
    if args.floor_margin_cm is not None and not 0.0 <= args.floor_margin_cm < float("inf"):
        parser.error("--floor_margin_cm is a height in centimetres, finite and >= 0, got %r" % args.floor_margin_cm)
    if args.dense and args.blend_space == "rot" and args.floor == "clamp":
        parser.error("--floor clamp does not go with --blend_space rot: the clamp moves joint positions, so the saved rotations would no "
                     "longer produce pred (--floor measure goes with every space)")
    if args.smooth is not None and not 1 <= args.smooth <= 31:
        parser.error("--smooth is the filter's half-width in frames: it has to lie in [1, 31] (2 H + 1 taps fit one wave), got %d"
                     % args.smooth)
    if args.dense and args.blend_space == "rot" and args.smooth is not None:
        parser.error("--smooth does not go with --blend_space rot: the filter runs on joint positions, so the saved rotations would not "
                     "be filtered with the positions (--rot_smooth H filters the rotations and lays the positions along them)")
    check_online(parser, args)
    if not args.dense:
        for flag in ("stride", "blend", "blend_space", "save_pred", "smooth", "smooth_order", "smooth_taper", "rot_smooth", "rot_smooth_order",
                     "rot_smooth_taper", "floor", "floor_contact_cm", "floor_margin_cm"):
            if getattr(args, flag) is not None:
                parser.error("--%s belongs to --infer --dense (sliding-window inference); without --dense nothing reads it" % flag)
        return
    if args.train:
        parser.error("--dense does not go with --train: it is an inference pass (training on the dense plan is not provided)")
    if not args.infer:
        parser.error("--dense goes with --infer only")
    if args.vis:
        parser.error("--dense does not go with --vis: it writes its skeletons with --save_pred instead")
    if args.stride is not None and not 1 <= args.stride <= Config.frame_no:
        parser.error("--stride has to lie in [1, %d] (frame_no): a larger one leaves frames between windows uncovered, got %d"
                     % (Config.frame_no, args.stride))
    if args.batch_size is not None and args.batch_size < 1:
        parser.error("--batch_size is the window minibatch of the dense pass: at least 1, got %d" % args.batch_size)


def check_frame_store(parser, args):
    """--window_jitter, --point_keep, --point_noise and --point_noise_v change what a training run is trained on: they go with --train,
    and the three that touch the points with a net that reads points."""
    noise = [flag for flag in ("point_noise", "point_noise_v") if getattr(args, flag) is not None]
    if not args.window_jitter and args.point_keep is None and not noise:
        return
    if args.point_keep is not None and not 0.0 < args.point_keep <= 1.0:          # (false for NaN as well)
        parser.error("--point_keep is the probability that a radar return is kept: it has to lie in (0, 1], got %r" % (args.point_keep,))
    for flag in noise:
        if not 0.0 < getattr(args, flag) < float("inf"):                         # (false for NaN as well)
            parser.error("--%s is the standard deviation of the jitter on a radar return: it has to be finite and > 0, got %r"
                         % (flag, getattr(args, flag)))
    if args.infer or not args.train:
        parser.error("--window_jitter, --point_keep, --point_noise and --point_noise_v go with --train only: evaluation runs on the "
                     "reference's test windows with the loader's packing")
    if args.point_keep is not None and args.network == "IMU_Net":
        parser.error("--point_keep does not go with --network IMU_Net: stage 1 reads no points (--window_jitter does)")
    if noise and args.network == "IMU_Net":
        parser.error("--%s does not go with --network IMU_Net: stage 1 reads no points (--window_jitter does)" % noise[0])


def check_pose_noise(parser, args):
    """--pose_noise_deg and --pose_noise_t perturb the head pose that Upper_Net and Lower_Net are given: they go with a run that gives
    them one as data."""
    given = [flag for flag in ("pose_noise_deg", "pose_noise_t") if getattr(args, flag) is not None]
    if not given:
        return
    for flag in given:
        if not 0.0 < getattr(args, flag) < float("inf"):                         # (false for NaN as well)
            parser.error("--%s is the standard deviation of the head-pose noise: it has to be finite and > 0, got %r"
                         % (flag, getattr(args, flag)))
    flag = given[0]
    if not (args.train or args.infer):
        parser.error("--%s goes with --train (--network Upper_Net / Lower_Net) or --infer: nothing else runs a net on a head pose" % flag)
    if args.network == "IMU_Net":
        parser.error("--%s does not go with --network IMU_Net: stage 1 is given no head pose, it estimates one" % flag)
    for ft in ("finetune_imu", "finetune_all"):
        if getattr(args, ft):
            parser.error("--%s cannot be combined with --%s: that run trains the head pose, and no gradient flows through the perturbation"
                         % (flag, ft))
    if args.vis:
        parser.error("--%s does not go with --vis" % flag)


def check_imu_noise(parser, args):
    """--imu_noise_* and --imu_bias_* perturb the samples IMU_Net reads: they go with a run in which one runs."""
    given = [flag for flag in IMU_NOISE_FLAGS if getattr(args, flag) is not None]
    if not given:
        return
    for flag in given:
        if not 0.0 < getattr(args, flag) < float("inf"):                         # (false for NaN as well)
            parser.error("--%s is a standard deviation of the IMU noise: it has to be finite and > 0, got %r" % (flag, getattr(args, flag)))
    flag = given[0]
    if not (args.train or args.infer):
        parser.error("--%s goes with --train or --infer: nothing else runs an IMU_Net" % flag)
    if args.vis:
        parser.error("--%s does not go with --vis" % flag)
    if args.gt_head_pose and not (args.train and args.network == "IMU_Net"):
        parser.error("--%s cannot be combined with --gt_head_pose: the head pose comes from the recording there and no IMU_Net runs" % flag)


def check_metrics(parser, args):
    """--metrics full belongs to a run whose evaluation pass compares skeletons: --infer, or stage 2 / stage 3 training."""
    if args.metrics != "full":
        return
    if not (args.train or args.infer):
        parser.error("--metrics full goes with --train or --infer (it adds figures to their evaluation pass)")
    if args.network == "IMU_Net":
        parser.error("--metrics full does not go with --network IMU_Net: stage 1 evaluates a head pose, there is no skeleton to align")


def check_upper_variant(parser, args):
    """--upper_variant names the Upper net of a run that has one; the options that train it in stage 3 know the plain UpperNet only."""
    if args.upper_variant is None:
        return
    if args.train and args.network == "IMU_Net":
        parser.error("--upper_variant does not go with --network IMU_Net: stage 1 runs no Upper_Net")
    if args.upper_variant == "wlocal":
        for flag in ("finetune_upper", "finetune_all"):
            if getattr(args, flag):
                parser.error("--upper_variant wlocal cannot be combined with --%s: stage 3 trains a plain UpperNet only (UpperNetwlocal "
                             "stays frozen there)" % flag)


def check_clip_grad_norm(parser, args):
    """--clip_grad_norm belongs to a training run and is a positive threshold (inf allowed: measure only)."""
    if args.clip_grad_norm is None:
        return
    if not args.clip_grad_norm > 0.0:                  # (false for NaN as well)
        parser.error("--clip_grad_norm is a gradient-norm threshold: it has to be > 0 (inf: measure only), got %r" % (args.clip_grad_norm,))
    if args.infer or not args.train:
        parser.error("--clip_grad_norm goes with --train only (it bounds the optimiser's step)")


def check_ema_decay(parser, args):
    """--ema_decay belongs to a training run and is a decay strictly between 0 and 1."""
    if args.ema_decay is None:
        return
    if not 0.0 < args.ema_decay < 1.0:                 # (false for NaN as well)
        parser.error("--ema_decay is the decay of the weight average: it has to lie in (0, 1), got %r" % (args.ema_decay,))
    if args.infer or not args.train:
        parser.error("--ema_decay goes with --train only (it averages the weights an optimiser updates)")


def check_lr_schedule(parser, args):
    """The --lr_* options belong to a training run; each belongs to the kinds that read it and lies in its range."""
    given = [f for f in ("lr_schedule", "lr_warmup", "lr_min_ratio", "lr_decay_steps", "lr_step_every", "lr_step_gamma")
             if getattr(args, f) is not None]
    if not given:
        return
    if args.infer or not args.train:
        parser.error("--%s goes with --train only (it schedules the optimiser's learning rate)" % given[0])
    for f in ("lr_warmup", "lr_decay_steps", "lr_step_every"):
        if getattr(args, f) is not None and getattr(args, f) < 1:
            parser.error("--%s is a number of optimiser steps: it has to be >= 1, got %r" % (f, getattr(args, f)))
    if args.lr_min_ratio is not None:
        if args.lr_schedule is None:
            parser.error("--lr_min_ratio is where --lr_schedule's decay ends; without --lr_schedule nothing decays")
        if not 0.0 <= args.lr_min_ratio < 1.0:         # (false for NaN as well)
            parser.error("--lr_min_ratio is a fraction of the learning rate: it has to lie in [0, 1), got %r" % (args.lr_min_ratio,))
    if args.lr_decay_steps is not None and args.lr_schedule not in ("cosine", "linear"):
        parser.error("--lr_decay_steps is the length of a cosine or linear decay: it goes with --lr_schedule cosine / linear only")
    for f in ("lr_step_every", "lr_step_gamma"):
        if getattr(args, f) is not None and args.lr_schedule != "step":
            parser.error("--%s belongs to --lr_schedule step only" % f)
    if args.lr_schedule == "step":
        for f in ("lr_step_every", "lr_step_gamma"):
            if getattr(args, f) is None:
                parser.error("--lr_schedule step needs --lr_step_every and --lr_step_gamma: --%s is missing" % f)
        if not 0.0 < args.lr_step_gamma <= 1.0:        # (false for NaN as well)
            parser.error("--lr_step_gamma is the factor of each decay: it has to lie in (0, 1], got %r" % (args.lr_step_gamma,))


def check_weight_decay(parser, args):
    """--weight_decay, --decay_mode and --no_decay_1d belong to a training run; the last two shape the first; W is finite and >= 0."""
    given = [f for f in ("weight_decay", "decay_mode") if getattr(args, f) is not None] + (["no_decay_1d"] if args.no_decay_1d else [])
    if not given:
        return
    if args.infer or not args.train:
        parser.error("--%s goes with --train only (it shapes the optimiser's weight decay)" % given[0])
    if args.weight_decay is None:
        parser.error("--%s shapes --weight_decay's decay; without --weight_decay the run keeps the reference's" % given[0])
    if not 0.0 <= args.weight_decay < float("inf"):    # (false for NaN as well)
        parser.error("--weight_decay is a decay strength: it has to be finite and >= 0, got %r" % (args.weight_decay,))


def check_finetune_upper(parser, args, world):
    """--finetune_upper fits one arrangement only; everything else is refused before any work starts.  (--gt_head_pose is fine: the
    head pose is not what is trained.)"""
    if not args.finetune_upper:
        if args.upper_lr is not None and not args.finetune_all:
            parser.error("--upper_lr is the Upper_Net's learning rate under --finetune_upper; without that flag the Upper_Net is frozen")
        return
    if not (args.train and args.network == "Lower_Net") or args.infer:
        parser.error("--finetune_upper goes with --train --network Lower_Net only (joint stage-3 training of Upper_Net and Lower_Net)")
    if world > 1:
        parser.error("--finetune_upper is not data parallel yet (WORLD_SIZE=%d): the Upper_Net gradients have no all-reduce" % world)
    if args.resume:
        parser.error("--finetune_upper cannot be combined with --resume yet: the Upper_Net's optimiser state is not part of a train state")


def check_imu_dropout(parser, args):
    """--imu_dropout belongs to a run that TRAINS an IMU_Net: stage 1, or stage 2 under --finetune_imu."""
    if args.imu_dropout is None:
        return
    if not 0.0 <= args.imu_dropout < 1.0:
        parser.error("--imu_dropout is a dropout rate: it has to lie in [0, 1), got %r" % (args.imu_dropout,))
    if args.finetune_all:
        return                      # (check_finetune_all has made sure that this run trains an IMU_Net)
    if args.infer or not (args.train and (args.network == "IMU_Net" or (args.network == "Upper_Net" and args.finetune_imu))):
        parser.error("--imu_dropout goes with --train --network IMU_Net or with --finetune_imu only (the runs that train an IMU_Net); "
                     "a frozen IMU_Net runs in eval mode, where dropout does nothing")


def check_finetune_all(parser, args, world):
    """--finetune_all fits one arrangement only; everything else is refused before any work starts."""
    if not args.finetune_all:
        return
    if args.finetune_imu or args.finetune_upper:
        parser.error("--finetune_all already means --finetune_imu and --finetune_upper for stage 3: give it alone")
    if not (args.train and args.network == "Lower_Net") or args.infer:
        parser.error("--finetune_all goes with --train --network Lower_Net only (stage 3 training IMU_Net, Upper_Net and Lower_Net together)")
    if args.gt_head_pose:
        parser.error("--finetune_all trains the IMU_Net, so it needs one; --gt_head_pose takes the head pose from the recording instead")
    if world > 1:
        parser.error("--finetune_all is not data parallel yet (WORLD_SIZE=%d): the IMU_Net and Upper_Net gradients have no all-reduce" % world)
    if args.resume:
        parser.error("--finetune_all cannot be combined with --resume yet: three optimiser states are not part of a train state")


def check_finetune(parser, args, world):
    """--finetune_imu fits one arrangement only; everything else is refused before any work starts."""
    check_upper_variant(parser, args)
    check_metrics(parser, args)
    check_finetune_all(parser, args, world)
    check_finetune_upper(parser, args, world)
    check_imu_dropout(parser, args)
    check_clip_grad_norm(parser, args)
    check_ema_decay(parser, args)
    check_lr_schedule(parser, args)
    check_weight_decay(parser, args)
    check_frame_store(parser, args)
    check_render(parser, args)
    check_dense(parser, args)
    check_pose_noise(parser, args)
    check_imu_noise(parser, args)
    check_breakdown(parser, args)
    if not args.finetune_imu:
        if args.imu_lr is not None and not args.finetune_all:
            parser.error("--imu_lr is the IMU_Net's learning rate under --finetune_imu; without that flag the IMU_Net is frozen")
        return
    if not (args.train and args.network == "Upper_Net"):
        parser.error("--finetune_imu goes with --train --network Upper_Net only (stage 3 trains the IMU_Net under --finetune_all, together with the Upper_Net)")
    if args.gt_head_pose:
        parser.error("--finetune_imu needs an IMU_Net to train; --gt_head_pose takes the head pose from the recording instead")
    if world > 1:
        parser.error("--finetune_imu is not data parallel yet (WORLD_SIZE=%d): the IMU_Net gradients have no all-reduce" % world)
    if args.resume:
        parser.error("--finetune_imu cannot be combined with --resume yet: the IMU_Net's optimiser state is not part of a train state")


def apply_overrides(args):
    both = (Config, ConfigDemo)
    if args.colab:
        ConfigDemo.colab = True
    if args.epochs is not None:
        Config.epochs = args.epochs
    if args.lr is not None:
        Config.lr = args.lr
    if args.batch_size is not None:
        Config.batch_size = args.batch_size
    if args.log_dir is not None:
        Config.Idx = args.log_dir
    for name, attr in (("device", "device"), ("load_IMU_path", "model_IMU_path"), ("load_Upper_path", "model_upper_path"),
                       ("load_Lower_path", "model_lower_path"), ("data_root", "data_root")):
        v = getattr(args, name)
        if v is not None:
            for c in both:
                setattr(c, attr, v)
    if args.gt_head_pose:
        for c in both:
            c.gt_head_pose = True
    Config.resume_path = args.resume
    Config.finetune_imu = bool(args.finetune_imu)
    Config.imu_lr = args.imu_lr
    Config.imu_dropout = args.imu_dropout
    Config.finetune_upper = bool(args.finetune_upper)
    Config.upper_lr = args.upper_lr
    Config.finetune_all = bool(args.finetune_all)
    Config.clip_grad_norm = args.clip_grad_norm
    Config.ema_decay = args.ema_decay
    Config.lr_schedule, Config.lr_warmup, Config.lr_min_ratio = args.lr_schedule, args.lr_warmup, args.lr_min_ratio
    Config.lr_decay_steps, Config.lr_step_every, Config.lr_step_gamma = args.lr_decay_steps, args.lr_step_every, args.lr_step_gamma
    Config.weight_decay, Config.decay_mode, Config.no_decay_1d = args.weight_decay, args.decay_mode, bool(args.no_decay_1d)
    Config.window_jitter = bool(args.window_jitter)
    Config.point_keep = args.point_keep
    Config.point_noise, Config.point_noise_v = args.point_noise, args.point_noise_v
    Config.seed = args.seed
    for c in both:
        c.pose_noise_deg, c.pose_noise_t = args.pose_noise_deg, args.pose_noise_t
    if args.pose_noise_deg is not None or args.pose_noise_t is not None:
        ConfigDemo.seed = args.seed                  # (--infer under the flags: the draws' seed)
    for c in both:
        for flag in IMU_NOISE_FLAGS:
            setattr(c, flag, getattr(args, flag))
    if any(getattr(args, flag) is not None for flag in IMU_NOISE_FLAGS):
        ConfigDemo.seed = args.seed                  # (likewise)
    for c in both:
        c.upper_variant = args.upper_variant or "global"
        c.metrics = args.metrics
    ConfigDemo.dense, ConfigDemo.stride, ConfigDemo.blend = bool(args.dense), args.stride, args.blend or "mean"
    ConfigDemo.save_pred, ConfigDemo.dense_batch_size, ConfigDemo.blend_space = args.save_pred, args.batch_size, args.blend_space
    ConfigDemo.smooth = None if args.smooth is None else (args.smooth, 2 if args.smooth_order is None else args.smooth_order,
                                                          args.smooth_taper or "gauss")
    ConfigDemo.rot_smooth = None if args.rot_smooth is None else (args.rot_smooth, 2 if args.rot_smooth_order is None else args.rot_smooth_order,
                                                                  args.rot_smooth_taper or "gauss")
    ConfigDemo.floor = None if args.floor is None else (args.floor, 6.0 if args.floor_contact_cm is None else args.floor_contact_cm,
                                                        0.0 if args.floor_margin_cm is None else args.floor_margin_cm)
    ConfigDemo.online = (args.lookahead or 0) if args.online else None
    if args.online and args.stride is None:          # (what a device with that budget has to compute)
        ConfigDemo.stride = max(1, min(ConfigDemo.online + 1, Config.frame_no // 2))
    ConfigDemo.one_euro = None if args.one_euro is None else (args.one_euro, 0.0 if args.one_euro_beta is None else args.one_euro_beta,
                                                              0.1 if args.one_euro_dcutoff is None else args.one_euro_dcutoff)
    ConfigDemo.breakdown = bool(args.breakdown)
    ConfigDemo.vis = bool(args.vis)
    ConfigDemo.render = None if args.render is None else (
        args.render, RENDER_SIZE if args.render_size is None else args.render_size,
        None if args.render_recordings is None else parse_recordings(args.render_recordings),
        RENDER_FPS if args.render_fps is None else args.render_fps)
    if args.imu_precision is not None:
        os.environ["MMEGO_IMU_PRECISION"] = args.imu_precision      # read by IMUNet.__init__
    if args.imu_train_precision is not None:
        os.environ["MMEGO_IMU_TRAIN_PRECISION"] = args.imu_train_precision


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_finetune(parser, args, int(os.environ.get("WORLD_SIZE", "1")))
    apply_overrides(args)
    if args.seed is not None:
        import numpy as np
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)          # PosePC pads / subsamples the point clouds with numpy's global generator
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and args.train:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        Config.device = "cuda:%d" % local
        Config.data_parallel = True
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))
    if args.train:
        if args.network == "IMU_Net":
            from Processor.Train.Train_IMU import MMEgo
            MMEgo().train_imu()
        if args.network == "Upper_Net":
            from Processor.Train.Train_Upper import MMEgo
            MMEgo().train_upper()
        if args.network == "Lower_Net":
            from Processor.Train.Train_Lower import MMEgo
            MMEgo().train_lower()
    elif args.infer:
        from Processor.Test.Demo_test import MMEgo
        processor = MMEgo()
        if args.vis:
            processor.eval_all_skeleton()
        elif args.dense:
            processor.eval_dense()
        else:
            processor.eval_model()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
