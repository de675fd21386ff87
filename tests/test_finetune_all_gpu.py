"""GPU: --finetune_all -- stage 3 training IMU_Net, Upper_Net and Lower_Net end to end on loss_lower + loss_upper.

The accumulating kinematics backward (mmego_head_fk_backward_extra) bit for bit against mmego_head_fk_backward_pose plus fp32 adds; one
step of train_step.StageStep("lower", finetune_upper=True, finetune_imu=True) against the CPU oracle's autograd through the three nets,
eager against graph replay, the refusals; and the command line on the synthetic data tree of tests/test_cli_gpu.py."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, set_lstm_dropout

pytestmark = pytest.mark.gpu

NOISE_GRAD = re.compile(r"(conv[123]\.bias|tcn\.2\.bias|residual\.0\.bias|attn\.bias|to_k\.bias|fusion\.attn\.weight)$")
LR, UPPER_LR, IMU_LR = 3e-5, 1e-5, 2e-5
GRAD_BAR = 2e-4
SENTINEL = 12345.678


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _guarded(value, dev):
    """-> (a contiguous copy of `value` on the device with 64 sentinel floats behind it, the sentinel view)."""
    n = value.numel()
    buf = torch.full((n + 64,), SENTINEL, dtype=torch.float32, device=dev)
    buf[:n] = value.reshape(-1).to(dev)
    return buf[:n].view(value.shape), buf[n:]


@pytest.mark.parametrize("which", [0, 1])
def test_head_fk_backward_extra_bit_for_bit(dev, which):
    """dy == dy0 + D, dRw == (dRw0 + S_R) + dR_add, dtw == (dtw0 + S_t) + dt_add with D, S_R, S_t from mmego_head_fk_backward_pose on
    the same inputs and the adds as fp32 torch adds on the device (torch.equal: that kernel is itself held to float64 by
    test_new_kernels_against_float64).  F = 1, 63, 64, 65, 203: one frame, a ragged last 64-thread workgroup, body rows f % B (Q2) with
    B not dividing 64.  Also without dR_add / dt_add, without dRw / dtw (dy only), sentinels behind every output, two runs equal bits;
    which = 0 (Upper head, what the step uses) and which = 1 (Lower head)."""
    from mmego_amd import hip
    ny, nslots, nrot = ((87, 15, 14), (42, 8, 6))[which]
    g = torch.Generator().manual_seed(500 + which)
    for B, T in ((1, 1), (3, 21), (8, 8), (5, 13), (7, 29)):
        F = B * T
        rnd = lambda *shape: torch.randn(*shape, generator=g)
        y, body, dj = rnd(F, ny).to(dev), (rnd(B, 20, 3) * 0.3).to(dev), rnd(F, nslots, 3).to(dev)
        Rw, tw = rnd(F, 3, 3).to(dev), rnd(F, 3).to(dev)
        q, jh, world = torch.empty(F, nrot, 3, 3, device=dev), torch.empty(F, nslots, 3, device=dev), torch.empty(F, nslots, 3, device=dev)
        hip.call("head_fk_forward", which, y, body, B, F, q, jh, Rw, tw, world, None, 0, None)
        dy0, dR0, dt0, dR_add, dt_add = rnd(F, ny), rnd(F, 3, 3), rnd(F, 3), rnd(F, 3, 3).to(dev), rnd(F, 3).to(dev)
        D, S_R, S_t = torch.empty(F, ny, device=dev), torch.empty(F, 3, 3, device=dev), torch.empty(F, 3, device=dev)
        hip.call("head_fk_backward_pose", which, y, body, B, F, dj, D, Rw, jh, S_R, S_t)
        want_dy = dy0.to(dev) + D
        for adds in (True, False):
            want_R, want_t = dR0.to(dev) + S_R, dt0.to(dev) + S_t
            if adds:
                want_R, want_t = want_R + dR_add, want_t + dt_add
            runs = []
            for _ in range(2):
                (dy, s0), (dR, s1), (dt, s2) = _guarded(dy0, dev), _guarded(dR0, dev), _guarded(dt0, dev)
                hip.call("head_fk_backward_extra", which, y, body, B, F, dj, dy, Rw, jh, dR, dt, dR_add if adds else None, dt_add if adds else None)
                torch.cuda.synchronize()
                for s in (s0, s1, s2):
                    assert bool((s == SENTINEL).all()), (F, adds)
                runs.append((dy.clone(), dR.clone(), dt.clone()))
            assert torch.equal(runs[0][0], want_dy), (F, adds, float((runs[0][0] - want_dy).abs().max()))
            assert torch.equal(runs[0][1], want_R), (F, adds, float((runs[0][1] - want_R).abs().max()))
            assert torch.equal(runs[0][2], want_t), (F, adds, float((runs[0][2] - want_t).abs().max()))
            for a, b in zip(*runs):
                assert torch.equal(a, b), (F, adds)
        # without dRw / dtw: dy only (joints_h is not needed then)
        dy, s0 = _guarded(dy0, dev)
        hip.call("head_fk_backward_extra", which, y, body, B, F, dj, dy, Rw, None, None, None, None, None)
        torch.cuda.synchronize()
        assert torch.equal(dy, want_dy) and bool((s0 == SENTINEL).all()), F
    # what the entry point cannot do is a bad argument, not a launch
    for bad in ((2, dy, Rw, jh, dR, dt, None, None), (which, dy, None, jh, dR, dt, None, None), (which, dy, Rw, jh, dR, None, None, None),
                (which, dy, Rw, None, dR, dt, None, None), (which, dy, Rw, None, None, None, dR_add, dt_add)):
        with pytest.raises(RuntimeError, match="bad argument"):
            hip.call("head_fk_backward_extra", bad[0], y, body, B, F, dj, *bad[1:])


def _hip_stage(dev, sd_imu, sd_up, sd_lo, batch, use_graph):
    from mmego_amd import nets
    from mmego_amd.train_step import StageStep
    himu = nets.IMUNet(15, 9, 512, 2, True, 0)
    himu.load_state_dict(sd_imu)
    himu = himu.to(dev).train()
    hup = nets.UpperNet()
    hup.load_state_dict(sd_up)
    hup = hup.to(dev).train()
    hlo = nets.LowerNet(64)
    hlo.load_state_dict(sd_lo)
    hlo = hlo.to(dev).train()
    hup.lstm_dropout = hlo.lstm_dropout = 0
    st = StageStep("lower", hlo, himu, upper_frozen=hup, lr=LR, use_graph=use_graph, finetune_upper=True, finetune_imu=True,
                   upper_lr=UPPER_LR, imu_lr=IMU_LR)
    x, imu, body, target = [v.to(dev) for v in batch]
    st.bind(x, imu, body, target)
    return st


def test_finetune_all_step_against_oracle(dev, monkeypatch):
    """B=4, T=8, N=128.  Oracle (fp32, CPU, one thread): IMU_Net(15, 9, 512, 2, True, 0)(train) -> Upper_Net(train) -> Lower_Net(train),
    nothing detached but Lower_Net's point input (a detached clone of the once-transformed points: the in-place second transform, Q1,
    would otherwise invalidate what Upper_Net's autograd saved -- and the step does not differentiate that path either), the HIP step's
    point selection, loss l1_sum(lower) + l1_sum(upper).  The bars of test_finetune_step_against_oracle and
    test_finetune_upper_step_against_oracle: both losses within 2e-5 relative; every gradient of each of the three nets within 2e-4 of
    that net's largest gradient; fc3 (Q7) without gradient; after the three Adam steps (Lower_Net at lr, Upper_Net at upper_lr, IMU_Net
    at imu_lr with weight decay 1e-3) the parameters as those tests compare them; graph replay == eager bit for bit over two steps;
    the arrangements the step does not fit are refused by name."""
    from mmego_amd import blocks
    from mmego_amd.train_step import ConcurrentStages, PipelinedStages, SharedImuStages, StageStep
    from oracle import nets as on
    from oracle import skeleton as sk
    from oracle import train as ot
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        B, T, N = 4, 8, 128
        torch.manual_seed(81)
        oimu = on.IMUNet(15, 9, 512, 2, True, 0).train()
        oup, olo = on.UpperNet().train(), on.LowerNet(64).train()
        set_lstm_dropout(oup, 0.0)
        set_lstm_dropout(olo, 0.0)
        sd_imu, sd_up, sd_lo = ({k: v.clone() for k, v in m.state_dict().items()} for m in (oimu, oup, olo))
        g = torch.Generator().manual_seed(82)
        x = torch.randn(B, T, N, 6, generator=g)
        imu = torch.randn(B, T, 20, 15, generator=g)
        body = torch.randn(B, 20, 3, generator=g) * 0.3
        target = torch.randn(B, T, 21, 3, generator=g)
        batch = (x, imu, body, target)

        st = _hip_stage(dev, sd_imu, sd_up, sd_lo, batch, use_graph=False)
        st.step()
        torch.cuda.synchronize()
        idx = st.net.last_select_idx.clone().cpu()

        h0, c0 = ot.zeros_state(B)
        R, t = oimu(imu)                                             # (no torch.no_grad(), no .detach())
        x1 = x.clone()
        up_o = oup(x1, h0, c0, body, R, t)[0]
        lo_o = olo(up_o, x1.detach().clone(), None, None, None, None, body, R, t, pin_select_idx=idx)[0]
        loss_lo = ot.l1_sum(lo_o, target[:, :, list(sk.LOWER_MAP)])
        loss_up = ot.l1_sum(up_o, target[:, :, list(sk.UPPER_MAP)])
        (loss_lo + loss_up).backward()

        print("three-net step: losses lower %.6f / %.6f, upper %.6f / %.6f" % (st.loss.item(), loss_lo.item(), st.upper_loss2[0].item(), loss_up.item()))
        assert abs(st.loss.item() - loss_lo.item()) < 2e-5 * abs(loss_lo.item()), (st.loss.item(), loss_lo.item())
        assert abs(st.upper_loss2[0].item() - loss_up.item()) < 2e-5 * abs(loss_up.item()), (st.upper_loss2[0].item(), loss_up.item())
        assert torch.allclose(st.last_pred.cpu(), lo_o.detach(), rtol=1e-4, atol=2e-5)
        assert torch.allclose(st.last_upper_pred.cpu(), up_o.detach(), rtol=1e-4, atol=2e-5)
        trio = (("imu", oimu, st.imu, IMU_LR, sd_imu), ("upper", oup, st.upper_frozen, UPPER_LR, sd_up), ("lower", olo, st.net, LR, sd_lo))
        failures = []
        for tag, o, h, _, _ in trio:
            po, ph = dict(o.named_parameters()), dict(h.named_parameters())
            flat = h.flat()
            scale = max(p.grad.abs().max().item() for p in po.values() if p.grad is not None)
            worst = 0.0
            for k in po:
                go = po[k].grad if po[k].grad is not None else torch.zeros_like(po[k])
                err = (flat.grad(ph[k]).detach().cpu() - go).abs().max().item()
                worst = max(worst, err)
                if not err < GRAD_BAR * scale:
                    failures.append((tag, k, err, scale))
            print("three-net step: %s gradients, worst error %.3e at scale %.3e (%.2e of it)" % (tag, worst, scale, worst / scale))
        assert not failures, failures
        assert oimu.fc3.weight.grad is None and oimu.fc3.bias.grad is None

        # the three Adam steps
        torch.optim.Adam(olo.parameters(), lr=LR).step()
        torch.optim.Adam(oup.parameters(), lr=UPPER_LR).step()
        torch.optim.Adam(oimu.parameters(), lr=IMU_LR, weight_decay=0.001).step()
        for tag, o, h, lr, sd in trio:
            n_bad = n_all = 0
            sd_o, sd_h = o.state_dict(), h.state_dict()
            for k, p in o.named_parameters():
                if NOISE_GRAD.search(k):
                    continue
                dp = (sd_h[k].cpu() - sd_o[k]).abs()
                assert dp.max().item() <= 2 * lr + 2e-6, (tag, k, dp.max().item())
                n_bad += int((dp > 2e-6).sum())
                n_all += dp.numel()
            print("three-net step: %s parameters, %d of %d moved by more than 2e-6" % (tag, n_bad, n_all))
            assert n_bad < 0.05 * n_all, (tag, n_bad, n_all)
            assert any(not torch.equal(sd_h[k].cpu(), sd[k]) for k, _ in o.named_parameters()), tag      # (really trained)
        for k in ("fc3.weight", "fc3.bias"):
            assert torch.equal(st.imu.state_dict()[k].cpu(), sd_imu[k]), k
        moved = [k for k, v in st.imu.state_dict().items() if not torch.equal(v.cpu(), sd_imu[k])]
        assert len(moved) == len(sd_imu) - 2, "every IMU_Net tensor but fc3 is trained"

        # graph replay == eager, bit for bit (two steps: the second replays the captured graph on updated weights)
        res = []
        for use_graph in (False, True):
            s2 = _hip_stage(dev, sd_imu, sd_up, sd_lo, batch, use_graph=use_graph)
            assert len(s2.optimisers()) == 3
            losses = []
            for _ in range(2):
                s2.step()
                losses.append((s2.loss.item(), s2.upper_loss2[0].item()))
            torch.cuda.synchronize()
            assert (s2.graph is not None) == use_graph
            three = (s2.net, s2.upper_frozen, s2.imu)
            res.append((losses, [v.clone() for m in three for v in (m.flat().flat_g, m.flat().flat_p)],
                        [b.clone() for m in three for b in m.buffers()], [m.seed_counter().clone() for m in three]))
        assert res[0][0] == res[1][0], (res[0][0], res[1][0])
        for i in (1, 2, 3):
            assert len(res[0][i]) == len(res[1][i])
            for a, b in zip(res[0][i], res[1][i]):
                assert torch.equal(a, b), i
        assert blocks.seq_xcd_errors() == 0

        # what the step does not fit is refused, by name
        hlo, hup, himu = s2.net, s2.upper_frozen, s2.imu
        both = dict(upper_frozen=hup, finetune_upper=True, finetune_imu=True)
        with pytest.raises(ValueError, match="finetune_upper"):
            StageStep("lower", hlo, None, **both)                                   # no IMU_Net to train
        R_d, t_d = torch.zeros(B, T, 3, 3, device=dev), torch.zeros(B, T, 3, device=dev)
        with pytest.raises(ValueError, match="recorded or shared head pose"):
            StageStep("lower", hlo, himu, pose=(R_d, t_d), **both)
        monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
        with pytest.raises(ValueError, match="not data parallel"):
            StageStep("lower", hlo, himu, process_group=object(), **both)
        monkeypatch.undo()
        with pytest.raises(ValueError, match="finetune_imu"):
            ConcurrentStages([s2])
        with pytest.raises(ValueError, match="finetune_imu"):
            PipelinedStages([s2], [None], None)
        with pytest.raises(ValueError, match="finetune_imu"):
            SharedImuStages(None, [s2], None)
        # ... and the Lower stage with finetune_imu alone stays refused
        with pytest.raises(ValueError, match="finetune_imu"):
            StageStep("lower", hlo, himu, upper_frozen=hup, finetune_imu=True)
    finally:
        torch.set_num_threads(threads)


def test_three_net_step_without_the_fused_loss_launch(dev, monkeypatch):
    """UpperNet._backward_impl(dl, dl_extra, pose_add) where the kinematics launch did not take the loss along (nets._FUSED_HEAD_LOSS
    off: l1_loss as a launch of its own, dl + dl_extra summed, mmego_head_fk_backward_pose, then pose_add by two accumulating copies)
    against the fused form (mmego_head_fk_loss_pose + mmego_head_fk_backward_extra) on the same step, B=4, T=8, N=128: each form
    really launches what it is said to, and both losses, the head pose's gradients that reach IMU_Net and every gradient of the three
    nets agree.  Both forms are fp32 evaluations of the same sums in another order (dy of a summed gradient against the sum of two
    dy's): the bar is the project's 2e-4 of the largest entry, as against the oracle."""
    from mmego_amd import nets
    from mmego_amd.plan import StepPlan
    B, T, N = 4, 8, 128
    torch.manual_seed(91)
    sd_imu, sd_up, sd_lo = ({k: v.clone() for k, v in m.state_dict().items()}
                            for m in (nets.IMUNet(15, 9, 512, 2, True, 0), nets.UpperNet(), nets.LowerNet(64)))
    g = torch.Generator().manual_seed(92)
    batch = (torch.randn(B, T, N, 6, generator=g), torch.randn(B, T, 20, 15, generator=g), torch.randn(B, 20, 3, generator=g) * 0.3,
             torch.randn(B, T, 21, 3, generator=g))
    got = {}
    for fused in (True, False):
        monkeypatch.setattr(nets, "_FUSED_HEAD_LOSS", fused)
        st = _hip_stage(dev, sd_imu, sd_up, sd_lo, batch, use_graph=False)
        st._body()
        torch.cuda.synchronize()
        names = [n for sg in StepPlan().record(st._body).segments for n, _ in sg.calls]
        assert names.count("head_fk_backward_extra") == (1 if fused else 0), names
        assert names.count("head_fk_loss_pose") == (2 if fused else 0) and names.count("head_fk_backward_pose") == (0 if fused else 2), names
        assert names.count("l1_loss") == (0 if fused else 2), names
        dR, dt = st.upper_frozen.pose_grads()
        got[fused] = dict(loss=(st.loss.item(), st.upper_loss2[0].item()), dR=dR.clone(), dt=dt.clone(), imu=st.imu.flat().flat_g.clone(),
                          upper=st.upper_frozen.flat().flat_g.clone(), lower=st.net.flat().flat_g.clone())
    monkeypatch.undo()
    for a, b in zip(got[True]["loss"], got[False]["loss"]):
        assert abs(a - b) < 2e-5 * abs(a), (a, b)
    for tag in ("dR", "dt", "imu", "upper", "lower"):
        a, b = got[True][tag], got[False][tag]
        scale, err = float(a.abs().max()), float((a - b).abs().max())
        print("three-net step, fused against unfused loss launch: %s %.3e at scale %.3e" % (tag, err, scale))
        assert scale > 0 and err < GRAD_BAR * scale, (tag, err, scale)


def test_cli_finetune_all_one_epoch(tmp_path):
    """main.py --train --network Lower_Net --finetune_all --epochs 1 --batch_size 4 --seed 5 --clip_grad_norm inf from saved random
    IMU_Net and Upper_Net checkpoints: the Lower_Net checkpoint and a file of the same name in IMU_Net/ and in Upper_Net/, all three
    trained (the two loaded nets differ from their checkpoints, Lower_Net from the seeded initialisation and its BatchNorm layers have
    counted minibatches), the loaded files as they were, one "Grad norm" line per net."""
    from test_cli_gpu import _make_dataset, _run
    from mmego_amd import nets
    data = str(tmp_path / "Sample_data")
    _make_dataset(data, np.random.default_rng(3))
    torch.manual_seed(2)
    imu_ck, up_ck = str(tmp_path / "imu.pth"), str(tmp_path / "upper.pth")
    start_imu, start_up = nets.IMUNet(15, 9, 512, 2, True, 0.1).state_dict(), nets.UpperNet().state_dict()
    torch.save(start_imu, imu_ck)
    torch.save(start_up, up_ck)
    start_imu, start_up = ({k: v.clone() for k, v in sd.items()} for sd in (start_imu, start_up))
    out_dir = str(tmp_path / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    out = _run(["--train", "--network", "Lower_Net", "--finetune_all", "--load_IMU_path", imu_ck, "--load_Upper_path", up_ck, "--data_root", data,
                "--epochs", "1", "--batch_size", "4", "--seed", "5", "--clip_grad_norm", "inf", "--upper_lr", "1e-4", "--imu_lr", "1e-4",
                "--device", "cuda:0", "--log_dir", "9161"], env)
    assert "epoch: 1" in out and "Average LowerBody Joint Localization Error" in out
    norms = re.findall(r"^Grad norm \((\w+)\): mean (\S+) max (\S+) clipped 0/(\d+) skipped 0$", out, flags=re.M)
    assert sorted(n[0] for n in norms) == ["IMU_Net", "Lower_Net", "Upper_Net"], out[-2000:]
    assert all(np.isfinite(float(n[1])) and float(n[1]) > 0 and int(n[3]) > 0 for n in norms), norms
    mdir = os.path.join(out_dir, "model", "9161")
    lo = [f for f in glob.glob(os.path.join(mdir, "epoch0_batch4frame*.pth")) if not f.endswith(".train_state.pth")]
    assert len(lo) == 1, os.listdir(mdir)
    name = os.path.basename(lo[0])
    im, up = os.path.join(mdir, "IMU_Net", name), os.path.join(mdir, "Upper_Net", name)
    assert os.path.exists(im) and os.path.exists(up), os.listdir(mdir)
    got_lo, got_im, got_up = (torch.load(f, map_location="cpu") for f in (lo[0], im, up))
    nets.LowerNet(64).load_state_dict(got_lo)
    nets.IMUNet(15, 9, 512, 2, True, 0).load_state_dict(got_im)
    nets.UpperNet().load_state_dict(got_up)
    for got in (got_lo, got_im, got_up):
        for k, v in got.items():
            assert bool(torch.isfinite(v.float()).all()), k
    for k in start_imu:
        assert torch.equal(got_im[k], start_imu[k]) == k.startswith("fc3."), k          # (fc3 is never trained, Q7)
    params = {k for k, _ in nets.UpperNet().named_parameters()}
    for k in start_up:
        if k in params and not NOISE_GRAD.search(k):
            assert not torch.equal(got_up[k], start_up[k]), k
    # Lower_Net is not loaded: --seed 5 seeds its initialisation (the trainer builds its IMU_Net first, then the Lower_Net)
    torch.manual_seed(5)
    nets.IMUNet(15, 9, 512, 2, True, 0)
    init_lo = nets.LowerNet(64).state_dict()
    assert any(not torch.equal(got_lo[k], init_lo[k]) for k, _ in nets.LowerNet(64).named_parameters())
    tracked = [v for k, v in got_lo.items() if k.endswith("num_batches_tracked")]
    assert tracked and all(int(v) > 0 for v in tracked), tracked
    # the checkpoints it loaded are as they were
    for path, start in ((imu_ck, start_imu), (up_ck, start_up)):
        after = torch.load(path, map_location="cpu")
        for k in start:
            assert torch.equal(after[k], start[k]), k
