"""GPU: --finetune_upper -- joint stage-3 training: Upper_Net trained through Lower_Net's input gradients (Train_Lower.py:195-196
without its .detach()) on the sum of the two stages' own L1(sum) losses.

One step of train_step.StageStep("lower", finetune_upper=True) against the CPU oracle's autograd through both nets, eager against
graph replay, the refusals, and the command line on the synthetic data tree of tests/test_cli_gpu.py."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, set_lstm_dropout

pytestmark = pytest.mark.gpu

NOISE_GRAD = re.compile(r"(conv[123]\.bias|tcn\.2\.bias|residual\.0\.bias|attn\.bias|to_k\.bias|fusion\.attn\.weight)$")
LR, UPPER_LR = 3e-5, 1e-5
GRAD_BAR = 2e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _hip_stage(dev, sd_up, sd_lo, batch, use_graph):
    from mmego_amd import nets
    from mmego_amd.train_step import StageStep
    hup = nets.UpperNet()
    hup.load_state_dict(sd_up)
    hup = hup.to(dev).train()
    hlo = nets.LowerNet(64)
    hlo.load_state_dict(sd_lo)
    hlo = hlo.to(dev).train()
    hup.lstm_dropout = hlo.lstm_dropout = 0
    st = StageStep("lower", hlo, None, upper_frozen=hup, lr=LR, use_graph=use_graph, finetune_upper=True, upper_lr=UPPER_LR)
    x, body, target, R = [v.to(dev) for v in batch]
    st.bind(x, None, body, target, R_gt=R)
    return st


def test_finetune_upper_step_against_oracle(dev, monkeypatch):
    """B=4, T=8, N=128, recorded head pose.  Oracle (fp32, CPU, one thread): Upper_Net(train) -> Lower_Net(train) without detach, loss
    l1_sum(lower) + l1_sum(upper); its Lower_Net gets a detached clone of the once-transformed points (the in-place second transform, Q1,
    would otherwise invalidate what Upper_Net's autograd saved) and the HIP step's point selection.  Both losses within 2e-5 relative;
    every gradient of either net within 2e-4 of that net's largest gradient; after the two Adam steps (Lower_Net at lr, Upper_Net at
    upper_lr) the parameters as test_finetune_step_against_oracle compares them; graph replay == eager bit for bit over two steps;
    the arrangements the option does not fit are refused by name."""
    from mmego_amd import blocks, nets, nets_local
    from mmego_amd.train_step import ConcurrentStages, PipelinedStages, SharedImuStages, StageStep
    from oracle import geometry as geo
    from oracle import nets as on
    from oracle import skeleton as sk
    from oracle import train as ot
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        B, T, N = 4, 8, 128
        torch.manual_seed(71)
        oup, olo = on.UpperNet().train(), on.LowerNet(64).train()
        set_lstm_dropout(oup, 0.0)
        set_lstm_dropout(olo, 0.0)
        sd_up = {k: v.clone() for k, v in oup.state_dict().items()}
        sd_lo = {k: v.clone() for k, v in olo.state_dict().items()}
        g = torch.Generator().manual_seed(72)
        x = torch.randn(B, T, N, 6, generator=g)
        body = torch.randn(B, 20, 3, generator=g) * 0.3
        target = torch.randn(B, T, 21, 3, generator=g)
        R = geo.rot6d_imu(torch.randn(B * T, 6, generator=g)).view(B, T, 3, 3).contiguous()
        batch = (x, body, target, R)

        st = _hip_stage(dev, sd_up, sd_lo, batch, use_graph=False)
        st.step()
        torch.cuda.synchronize()
        idx = st.net.last_select_idx.clone().cpu()

        h0, c0 = ot.zeros_state(B)
        t = target[:, :, 20].contiguous()
        x1 = x.clone()
        up_o = oup(x1, h0, c0, body, R, t)[0]
        lo_o = olo(up_o, x1.detach().clone(), None, None, None, None, body, R, t, pin_select_idx=idx)[0]
        loss_lo = ot.l1_sum(lo_o, target[:, :, list(sk.LOWER_MAP)])
        loss_up = ot.l1_sum(up_o, target[:, :, list(sk.UPPER_MAP)])
        (loss_lo + loss_up).backward()

        print("joint step: losses lower %.6f / %.6f, upper %.6f / %.6f" % (st.loss.item(), loss_lo.item(), st.upper_loss2[0].item(), loss_up.item()))
        assert abs(st.loss.item() - loss_lo.item()) < 2e-5 * abs(loss_lo.item()), (st.loss.item(), loss_lo.item())
        assert abs(st.upper_loss2[0].item() - loss_up.item()) < 2e-5 * abs(loss_up.item()), (st.upper_loss2[0].item(), loss_up.item())
        assert torch.allclose(st.last_pred.cpu(), lo_o.detach(), rtol=1e-4, atol=2e-5)
        assert torch.allclose(st.last_upper_pred.cpu(), up_o.detach(), rtol=1e-4, atol=2e-5)
        for tag, o, h in (("upper", oup, st.upper_frozen), ("lower", olo, st.net)):
            po, ph = dict(o.named_parameters()), dict(h.named_parameters())
            flat = h.flat()
            scale = max(p.grad.abs().max().item() for p in po.values() if p.grad is not None)
            worst = 0.0
            for k in po:
                go = po[k].grad if po[k].grad is not None else torch.zeros_like(po[k])
                err = (flat.grad(ph[k]).detach().cpu() - go).abs().max().item()
                worst = max(worst, err)
                assert err < GRAD_BAR * scale, (tag, k, err, scale)
            print("joint step: %s gradients, worst error %.3e at scale %.3e (%.2e of it)" % (tag, worst, scale, worst / scale))

        # the two Adam steps
        torch.optim.Adam(olo.parameters(), lr=LR).step()
        torch.optim.Adam(oup.parameters(), lr=UPPER_LR).step()
        for tag, o, h, lr, sd in (("upper", oup, st.upper_frozen, UPPER_LR, sd_up), ("lower", olo, st.net, LR, sd_lo)):
            n_bad = n_all = 0
            sd_o, sd_h = o.state_dict(), h.state_dict()
            for k, p in o.named_parameters():
                if NOISE_GRAD.search(k):
                    continue
                dp = (sd_h[k].cpu() - sd_o[k]).abs()
                assert dp.max().item() <= 2 * lr + 2e-6, (tag, k, dp.max().item())
                n_bad += int((dp > 2e-6).sum())
                n_all += dp.numel()
            print("joint step: %s parameters, %d of %d moved by more than 2e-6" % (tag, n_bad, n_all))
            assert n_bad < 0.05 * n_all, (tag, n_bad, n_all)
            assert any(not torch.equal(sd_h[k].cpu(), sd[k]) for k, _ in o.named_parameters()), tag      # (really trained)

        # graph replay == eager, bit for bit (two steps: the second replays the captured graph on updated weights)
        res = []
        for use_graph in (False, True):
            s2 = _hip_stage(dev, sd_up, sd_lo, batch, use_graph=use_graph)
            losses = []
            for _ in range(2):
                s2.step()
                losses.append((s2.loss.item(), s2.upper_loss2[0].item()))
            torch.cuda.synchronize()
            assert (s2.graph is not None) == use_graph
            res.append((losses, [v.clone() for m in (s2.net, s2.upper_frozen) for v in (m.flat().flat_g, m.flat().flat_p)],
                        [b.clone() for m in (s2.net, s2.upper_frozen) for b in m.buffers()],
                        [m.seed_counter().clone() for m in (s2.net, s2.upper_frozen)]))
        assert res[0][0] == res[1][0], (res[0][0], res[1][0])
        for i in (1, 2, 3):
            assert len(res[0][i]) == len(res[1][i])
            for a, b in zip(res[0][i], res[1][i]):
                assert torch.equal(a, b), i
        assert blocks.seq_xcd_errors() == 0

        # what the option does not fit is refused, by name
        hup, hlo = s2.upper_frozen, s2.net
        with pytest.raises(ValueError, match="finetune_upper"):
            StageStep("upper", hup, None, finetune_upper=True)
        with pytest.raises(ValueError, match="finetune_upper"):
            StageStep("lower", hlo, None, finetune_upper=True)
        with pytest.raises(ValueError, match="finetune_upper"):
            StageStep("lower", hlo, None, upper_frozen=nets_local.UpperNetwlocal().to(dev), finetune_upper=True)
        with pytest.raises(ValueError, match="finetune_upper"):
            StageStep("lower", hlo, None, upper_frozen=hup, finetune_upper=True, finetune_imu=True)
        pg = object()
        monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
        with pytest.raises(ValueError, match="finetune_upper"):
            StageStep("lower", hlo, None, upper_frozen=hup, finetune_upper=True, process_group=pg)
        monkeypatch.undo()
        with pytest.raises(ValueError, match="finetune_upper"):
            ConcurrentStages([s2])
        with pytest.raises(ValueError, match="finetune_upper"):
            PipelinedStages([s2], [None], None)
        with pytest.raises(ValueError, match="finetune_upper"):
            SharedImuStages(None, [s2], None)
        # ... and the plain Lower stage beside it still refuses what it refused
        with pytest.raises(ValueError, match="finetune_imu"):
            StageStep("lower", hlo, None, upper_frozen=hup, finetune_imu=True)
    finally:
        torch.set_num_threads(threads)


def test_cli_finetune_upper_one_epoch(tmp_path):
    """main.py --train --network Lower_Net --finetune_upper --epochs 1 --seed 0 from a saved random Upper_Net checkpoint, recorded head
    pose: both checkpoints written and loadable, the Upper_Net's weights moved, the logged losses finite; the same command without the
    flag writes no Upper_Net folder and leaves the checkpoint it loaded alone."""
    from test_cli_gpu import _make_dataset, _run
    from mmego_amd import nets
    data = str(tmp_path / "Sample_data")
    _make_dataset(data, np.random.default_rng(3))
    torch.manual_seed(2)
    up_ck = str(tmp_path / "upper.pth")
    start = nets.UpperNet().state_dict()
    torch.save(start, up_ck)
    start = {k: v.clone() for k, v in start.items()}
    out_dir = str(tmp_path / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    common = ["--train", "--network", "Lower_Net", "--load_Upper_path", up_ck, "--gt_head_pose", "--data_root", data, "--epochs", "1",
              "--batch_size", "3", "--device", "cuda:0", "--seed", "0"]
    out = _run(common + ["--finetune_upper", "--upper_lr", "1e-4", "--log_dir", "9151"], env)
    assert "epoch: 1" in out and "Average LowerBody Joint Localization Error" in out
    mdir = os.path.join(out_dir, "model", "9151")
    lo = [f for f in glob.glob(os.path.join(mdir, "epoch0_batch3frame*.pth")) if not f.endswith(".train_state.pth")]
    up = glob.glob(os.path.join(mdir, "Upper_Net", "epoch0_batch3frame*.pth"))
    assert len(lo) == 1 and len(up) == 1, (os.listdir(mdir))
    assert os.path.basename(lo[0]) == os.path.basename(up[0])
    nets.LowerNet(64).load_state_dict(torch.load(lo[0], map_location="cpu"))
    got = torch.load(up[0], map_location="cpu")
    nets.UpperNet().load_state_dict(got)
    assert got.keys() == start.keys()
    params = {k for k, _ in nets.UpperNet().named_parameters()}
    for k in start:
        assert bool(torch.isfinite(got[k].float()).all()), k
        if k in params and not NOISE_GRAD.search(k):
            assert not torch.equal(got[k], start[k]), k
    log = open(os.path.join(out_dir, "report", "9151", "log-loss.txt")).read().split()
    assert np.isfinite(float(log[1]))
    # without the flag: the Upper_Net is frozen -- nothing saved for it, the loaded checkpoint as it was
    out = _run(common + ["--log_dir", "9152"], env)
    assert "epoch: 1" in out
    assert not os.path.exists(os.path.join(out_dir, "model", "9152", "Upper_Net"))
    after = torch.load(up_ck, map_location="cpu")
    for k in start:
        assert torch.equal(after[k], start[k]), k
