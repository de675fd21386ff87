"""Run-time configuration singletons, mutated by main.py's argparse exactly like the reference's
Config/config.py:11-70 and Config/config_demo.py:11-60 (class attributes used as flags; CLI > defaults).
"""
import os

import numpy as np
import torch

from . import skeleton as sk

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDER_SIZE, RENDER_FPS = 256, 10      # --render_size's and --render_fps's defaults, and what --vis draws at
# --imu_noise_* / --imu_bias_*: the six flags and configuration attributes, in the order of mmego_imu_jitter's sigmas
IMU_NOISE_FLAGS = ("imu_noise_rot_deg", "imu_noise_acc", "imu_noise_gyro", "imu_bias_rot_deg", "imu_bias_acc", "imu_bias_gyro")


def _default_device():
    return "cuda:0" if torch.cuda.is_available() else "cpu"


def _pretrained(*parts):
    root = os.environ.get("MMEGO_PRETRAINED_ROOT", os.path.join(_REPO, "Resource", "Pretrained_model"))
    return os.path.join(root, *parts)


class _Common:
    pb = 10
    colab = False
    frame_no = sk.FRAMES
    pc_no = sk.POINTS
    lower_pc_no = sk.LOWER_POINTS
    joint_num_all, joint_num_upper, joint_num_lower = sk.JOINTS_ALL, sk.JOINTS_UPPER, sk.JOINTS_LOWER
    num_action = 13
    IMU_used = True
    IMU_pretrained = Upper_pretrained = Lower_pretrained = False
    device = _default_device()
    skeleton_all = np.asarray(sk.BONES_ALL)
    skeleton_upper_body = np.asarray(sk.BONES_UPPER)
    skeleton_lower_body = np.asarray(sk.BONES_LOWER)
    kinect_upper_gragh = list(sk.GCN_EDGES)          # (sic) the reference's spelling
    kinect_joint_selection = list(sk.KINECT_SELECTION)
    upper_joint_map, lower_joint_map, hand_joint_map = list(sk.UPPER_MAP), list(sk.LOWER_MAP), list(sk.HAND_MAP)
    model_IMU_path = _pretrained("IMU_Net", "epoch173_batch20frame20lr3e-05.pth")
    model_upper_path = _pretrained("Upper_Net", "epoch451_batch20frame20lr3e-05.pth")
    model_lower_path = _pretrained("Lower_Net", "epoch161_batch20frame20lr0.0003.pth")
    dataset_random_seed = 1
    data_root = os.environ.get("MMEGO_DATA_ROOT", os.path.join(_REPO, "Resource", "Sample_data"))
    # Not in the reference: the shipped snapshot lacks the IMU_Net checkpoint (.MISSING_LARGE_BLOBS), so the head pose
    # can be taken from the recording instead (R = loader R_R0R, t = ground-truth head joint).
    gt_head_pose = False
    data_parallel = False       # set by main.py when launched under torch.distributed.run
    finetune_upper = False      # --finetune_upper: stage 3 trains the Upper_Net too (train_step.StageStep)
    finetune_all = False        # --finetune_all: stage 3 trains IMU_Net, Upper_Net and Lower_Net together (train_step.StageStep)
    upper_lr = None             # --upper_lr: its learning rate (None: lr)
    imu_dropout = None          # --imu_dropout: nn.LSTM(dropout=P) of the IMU_Net that is trained (None: 0, as the reference's stage 1)
    upper_variant = "global"    # --upper_variant: the class behind "Upper_Net" -- "global" (UpperNet) or "wlocal" (UpperNetwlocal, anchor branch)
    window_jitter = False       # --window_jitter: every epoch moves each training window to a valid start within +-(frame_no-1) frames (data.FrameStore)
    point_keep = None           # --point_keep: clouds re-packed on the device per minibatch, each return kept with this probability (None: the loader's packing)
    point_noise = None          # --point_noise: metres, standard deviation of the jitter the device packer adds to x, y, z of every kept return per minibatch; r follows (None: none)
    point_noise_v = None        # --point_noise_v: the same on the Doppler velocity, in the recordings' units (None: none)
    pose_noise_deg = None       # --pose_noise_deg: degrees per axis, standard deviation of the random rotation vector applied to every frame's head pose (None: none)
    pose_noise_t = None         # --pose_noise_t: metres per component, standard deviation of the random shift of every frame's head position (None: none)
    imu_noise_rot_deg = None    # --imu_noise_rot_deg: degrees per axis, white rotation noise on the orientation of every IMU sample IMU_Net reads (None: none)
    imu_noise_acc = None        # --imu_noise_acc: white noise per accelerometer component, in the recordings' units (None: none)
    imu_noise_gyro = None       # --imu_noise_gyro: the same on the gyroscope (None: none)
    imu_bias_rot_deg = None     # --imu_bias_rot_deg: degrees per axis, one rotation per window applied to all its samples' orientations (None: none)
    imu_bias_acc = None         # --imu_bias_acc: one offset per window and accelerometer component (None: none)
    imu_bias_gyro = None        # --imu_bias_gyro: the same on the gyroscope (None: none)
    seed = None                 # --seed, as main.py got it (None: 0 for what FrameStore draws)
    clip_grad_norm = None       # --clip_grad_norm: every trained net's gradient is clipped to this global norm ahead of its Adam step (None: off)
    lr_schedule = None          # --lr_schedule: cosine | linear | step; every trained net's rate follows it inside its Adam launch (None: constant)
    lr_warmup = None            # --lr_warmup: optimiser steps of linear warm-up (None: none)
    lr_min_ratio = None         # --lr_min_ratio: the decay's end as a fraction of lr (None: 0)
    lr_decay_steps = None       # --lr_decay_steps: the span of a cosine / linear decay (None: the rest of the run)
    lr_step_every = None        # --lr_step_every, --lr_step_gamma: the step decay
    lr_step_gamma = None
    ema_decay = None            # --ema_decay: every trained net keeps a weight average at this decay; evaluation uses it (None: off)
    weight_decay = None         # --weight_decay: the decay of every net the run trains (None: the reference's, IMU_Net 1e-3 and the others 0)
    decay_mode = None           # --decay_mode: l2 (coupled, the reference's) | adamw (decoupled, follows the scheduled rate) (None: l2)
    no_decay_1d = False         # --no_decay_1d: biases, BatchNorm scales and shifts and LSTM biases do not decay


class Config(_Common):
    Idx = 1001
    epochs = 600
    lr = 3e-5
    batch_size = 20


class ConfigDemo(_Common):
    Idx = 1
    batch_per_action = 3
    dense = False               # --dense: sliding-window inference over whole recordings (dense.dense_infer)
    stride = None               # --stride: frames between window starts (None: frame_no // 2)
    blend = "mean"              # --blend: mean or triangle
    blend_space = None          # --blend_space: joints, bones or rot (None: joints, without the bone-length figures)
    smooth = None               # --smooth H [--smooth_order D --smooth_taper T]: (H, D, T), the dense pass's temporal filter (None: off)
    rot_smooth = None           # --rot_smooth H [--rot_smooth_order D --rot_smooth_taper T]: (H, D, T), the filter of the blended rotations (None: off)
    online = None               # --online [--lookahead L]: L, the latency budget in frames of the causal window cover (None: the offline cover)
    one_euro = None             # --one_euro FC [--one_euro_beta B --one_euro_dcutoff DC]: (FC, B, DC), the dense pass's causal filter (None: off)
    floor = None                # --floor M [--floor_contact_cm H --floor_margin_cm C]: (M, H, C), the dense pass's floor figures / clamp (None: off)
    save_pred = None            # --save_pred: .npz of the per-frame skeletons
    dense_batch_size = None     # --batch_size under --dense: windows per minibatch (None: 64)
    render = None               # --render DIR [--render_size PX --render_recordings LIST --render_fps N]: (DIR, PX, recordings or None, N) (None: off)
    vis = False                 # --vis: the loader keeps the per-frame clouds, as under --dense (Evaluator.eval_all_skeleton draws them)
