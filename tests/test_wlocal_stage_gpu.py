"""GPU: UpperNetwlocal as a full member of the training stages -- its head-pose gradients (d loss / d R, d loss / d t) against the float64
CPU oracle, what stays as it was for a detached pose, the --finetune_imu step around it against the fp32 oracle, the Lower stage behind a
frozen one, the step engines around both, and the command line (--upper_variant wlocal) on the synthetic tree of tests/test_cli_gpu.py.

Bars: gradients within GRAD_BAR = 2e-4 of the largest gradient of their net (tests/test_input_grads_gpu.py, tests/test_finetune_gpu.py; the
first-step bar of test_hip_local.test_train_upper_wlocal is the same figure), joints rtol 1e-4 / atol 2e-5, loss 2e-5 relative, the Adam
check of test_finetune_step_against_oracle.

Precondition of every comparison with an oracle, asserted first: the two sides group the SAME points around every anchor (the index sets
of last_group_idx).  The selection is discrete: a differing set is a different function of the pose, not a rounding error."""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import step_helpers
from conftest import GOLDEN, ROOT, set_lstm_dropout
from oracle import geometry as geo
from oracle import nets as on
from oracle import skeleton as sk
from oracle import train as ot
from step_helpers import entry_points
from test_input_grads_gpu import _batch, _rel_err

pytestmark = pytest.mark.gpu

GRAD_BAR = 2e-4
NOISE_GRAD = re.compile(r"(conv[123]\.bias|tcn\.2\.bias|residual\.0\.bias|attn\.bias|to_k\.bias|fusion\.attn\.weight)$")
LR, IMU_LR = 3e-5, 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _same_groups(h_idx, o_idx, tag):
    """The precondition: per frame and anchor the same SET of 8 points on both sides."""
    a = torch.sort(h_idx.detach().cpu().reshape(-1, 27, 8), dim=-1).values
    b = torch.sort(o_idx.detach().cpu().reshape(-1, 27, 8), dim=-1).values
    differ = int((a != b).any(-1).sum())
    assert differ == 0, (tag, "%d of %d frame-anchor pairs group different points: another data seed, not a wider bar" % (differ, a.shape[0] * 27))


def _pair(dev, seed):
    """The oracle in float64 and the HIP net with the same weights, train mode, LSTM dropout off on both sides, the pose opted in."""
    from mmego_amd import nets_local
    torch.manual_seed(seed)
    o = on.UpperNetwlocal().train()
    h = nets_local.UpperNetwlocal().to(dev).train()
    h.load_state_dict({k: v.to(dev) for k, v in o.state_dict().items()})
    set_lstm_dropout(o, 0.0)
    set_lstm_dropout(h, 0.0)
    h.lstm_dropout = 0
    h.differentiable_inputs = True
    return o.double(), h


def _oracle_grads(o, x, body, R, t, target, monkeypatch):
    """float64 CPU oracle with both pose tensors requiring grad -> (joints, dR, dt, {name: parameter gradient}, group indices).
    (The oracle's anchor grid is an fp32 constant: handed to the float64 run as the same values in float64.)"""
    B = x.shape[0]
    grid32 = geo.anchor_grid
    monkeypatch.setattr(geo, "anchor_grid", lambda: grid32().double())
    Rd, td = R.double().requires_grad_(), t.double().requires_grad_()
    h0, c0 = [v.double() for v in ot.zeros_state(B)]
    for p in o.parameters():
        p.grad = None
    l = o(x.double().clone(), h0, c0, h0, c0, body.double(), Rd, td)[0]
    ot.l1_sum(l, target.double()).backward()
    return l.detach(), Rd.grad, td.grad, {k: p.grad for k, p in o.named_parameters()}, o.module2.last_group_idx.clone()


def _hip_grads(h, dev, x, body, R, t, target, need_R=True, need_t=True):
    B = x.shape[0]
    Rh, th = R.to(dev).requires_grad_(need_R), t.to(dev).requires_grad_(need_t)
    h0, c0 = [v.to(dev) for v in ot.zeros_state(B)]
    for p in h.parameters():
        p.grad = None
    l = h(x.to(dev).clone(), h0, c0, h0, c0, body.to(dev), Rh, th)[0]
    idx = h.last_group_idx.clone()
    (l - target.to(dev)).abs().sum().backward()
    torch.cuda.synchronize()
    return l.detach(), Rh.grad, th.grad, {k: p.grad.clone() for k, p in h.named_parameters()}, idx


# (N, orthonormal R, R requires grad, t requires grad, zero-padded points)
POSE_CASES = [
    (128, True, True, True, False),
    (128, False, True, True, False),
    (128, True, True, False, False),
    (128, True, False, True, False),
    (64, False, True, True, False),
    (96, True, True, True, False),           # _local_fusable(96) is False: the anchor branch on the launch chain (anchor_group_backward)
    (128, False, True, True, True),
]


@pytest.mark.parametrize("case", range(len(POSE_CASES)), ids=["N%d-%s-%s%s%s" % (c[0], "orth" if c[1] else "pert", "R" if c[2] else "", "t" if c[3] else "",
                                                                                  "-padded" if c[4] else "") for c in POSE_CASES])
def test_wlocal_head_pose_gradients_against_oracle(dev, case, monkeypatch):
    """B=2, T=4, train mode, loss L1(sum) on the 15 joints, through the opt-in autograd path (differentiable_inputs = True).  N = 64 and 128
    (the fused anchor kernels: anchor_scatter), N = 96 (the launch chain); orthonormal R and R perturbed by 1e-2 (the head-frame share must
    come from the untransformed points); only R / only t / both; one zero-padded batch.  Joints, dR, dt and EVERY parameter gradient: the
    offsets' gradient reaches PointNet through the head-frame transform's input only, not through a parameter, so the parameter gradients
    check that asking for the pose gradients moved nothing else."""
    B, T = 2, 4
    N, orth, need_R, need_t, padded = POSE_CASES[case]
    o, h = _pair(dev, 11)
    x, body, R, t, target = _batch(300 + case, B, T, N, orth, padded)
    lo, dRo, dto, po, idx_o = _oracle_grads(o, x, body, R, t, target, monkeypatch)
    lh, dRh, dth, ph, idx_h = _hip_grads(h, dev, x, body, R, t, target, need_R, need_t)
    tag = POSE_CASES[case]
    _same_groups(idx_h, idx_o, tag)
    assert h._local_fusable(N) == (N != 96) and h._local_was_fused == (N != 96), tag
    print("case", tag, "joints max err %.3e" % float((lh.double().cpu() - lo).abs().max()))
    assert torch.allclose(lh.cpu(), lo.float(), rtol=1e-4, atol=2e-5), (tag, float((lh.double().cpu() - lo).abs().max()))
    assert (dRh is not None) == need_R and (dth is not None) == need_t, tag
    if need_R:
        assert dRh.shape == R.shape and dRh.dtype == torch.float32
        err, scale = _rel_err(dRh, dRo)
        print("   dR max err %.3e at scale %.3e (%.2e of it)" % (err, scale, err / scale))
        assert err < GRAD_BAR * scale, (tag, "dR", err, scale)
    if need_t:
        assert dth.shape == t.shape and dth.dtype == torch.float32
        err, scale = _rel_err(dth, dto)
        print("   dt max err %.3e at scale %.3e (%.2e of it)" % (err, scale, err / scale))
        assert err < GRAD_BAR * scale, (tag, "dt", err, scale)
    scale = max(float(g.abs().max()) for g in po.values() if g is not None)
    worst = ("", 0.0)
    for k, go in po.items():
        go = go if go is not None else torch.zeros_like(dict(o.named_parameters())[k])
        err = float((ph[k].double().cpu() - go).abs().max())
        worst = max(worst, (k, err), key=lambda v: v[1])
    print("   parameter gradients: worst %s %.3e at scale %.3e (%.2e of it)" % (worst[0], worst[1], scale, worst[1] / scale))
    for k, go in po.items():
        go = go if go is not None else torch.zeros_like(dict(o.named_parameters())[k])
        err = float((ph[k].double().cpu() - go).abs().max())
        assert err < GRAD_BAR * scale, (tag, k, err, scale)


def test_wlocal_default_refuses_and_unused_pose_gradients_cost_nothing(dev):
    """Without the opt-in a pose that requires grad raises.  The recorded launches of a forward + backward without pose_grad are the
    parent's (tests/golden/step_structure.json, `upper_wlocal`: the step's copy of the recorded head joint in front, its Adam launch
    behind), with and without the fused loss launch; pose_grad=True adds only mmego_transform2h_backward at the end and swaps
    head_fk_loss / head_fk_backward for their _pose forms; no extra buffer is kept without it; two runs give the same bits, and the
    parameter gradients do not depend on whether the pose asked for its own."""
    from mmego_amd import nets_local
    from mmego_amd.train_step import StageStep
    B, T, N = step_helpers.B, step_helpers.T, step_helpers.N
    torch.manual_seed(5)
    net = nets_local.UpperNetwlocal().to(dev).train()
    x, _, body, target, R = step_helpers.batch(dev)
    t = target[:, :, 20].contiguous()
    h0 = torch.zeros(6, B, 64, device=dev)
    assert net.differentiable_inputs is False
    for name in ("R", "t"):
        a = dict(R=R.clone(), t=t.clone())
        a[name].requires_grad_()
        with pytest.raises(NotImplementedError, match="input gradients"):
            net(x.clone(), h0, h0, h0, h0, body, a["R"], a["t"])
    with pytest.raises(ValueError, match="stash"):
        with torch.no_grad():
            net._forward_impl(x.clone(), h0, h0, h0, h0, body, R, t, stash=False, pose_grad=True)

    # the launches
    st = StageStep("upper", net, None, lr=3e-5, use_graph=False)
    st.bind(x, None, body, target, R_gt=R)
    st.step()                                                       # (sizes the arenas, the loss scratch and the optimiser)
    torch.cuda.synchronize()
    assert net._pose is None and not any(net.arena("train").has(k) for k in ("pts_raw", "dR", "dt", "m0.dy0"))
    with pytest.raises(RuntimeError, match="pose_grads"):
        net.pose_grads()
    s = st.static
    dl = torch.zeros(B, T, 15, 3, device=dev)

    def body_of(pose_grad, hook):
        def run():
            net.loss_hook = (s["target"], st.jmap, st.loss2, 1.0) if hook else None
            try:
                with torch.no_grad():
                    net._forward_impl(s["x"], h0, h0, h0, h0, body, R, t, stash=True, x_src=s["x_src"], pose_grad=pose_grad)
                    net._backward_impl(dl)
            finally:
                net.loss_hook = None
        return run
    parent = json.load(open(os.path.join(GOLDEN, "step_structure.json")))["upper_wlocal"]
    assert len(parent["segments"]) == 1
    want = parent["segments"][0]["calls"]
    assert want[0] == "copy2d" and want[-1] == "adam_step"
    plain = entry_points(body_of(False, True))
    assert plain == want[1:-1], [(i, a, b) for i, (a, b) in enumerate(zip(plain, want[1:-1])) if a != b][:5]
    assert entry_points(st.step) == want
    posed = entry_points(body_of(True, True))
    assert posed == [{"head_fk_loss": "head_fk_loss_pose"}.get(n, n) for n in plain] + ["transform2h_backward"]
    assert plain.count("head_fk_loss") == 1
    plain_u, posed_u = entry_points(body_of(False, False)), entry_points(body_of(True, False))
    assert plain_u.count("head_fk_forward") == 1 and plain_u.count("head_fk_backward") == 1 and "head_fk_loss" not in plain_u
    assert posed_u == [{"head_fk_backward": "head_fk_backward_pose"}.get(n, n) for n in plain_u] + ["transform2h_backward"]

    # the bits: through the opt-in autograd path, twice with and once without the pose's gradients
    net.differentiable_inputs = True
    net.lstm_dropout = 0
    state = {k: v.clone() for k, v in net.state_dict().items()}
    xb, bodyb, Rb, tb, targetb = _batch(200, 2, 4, N, False, True)
    runs = []
    for need in (True, True, False):
        net.load_state_dict(state)
        runs.append(_hip_grads(net, dev, xb, bodyb, Rb, tb, targetb, need, need))
    (l0, dR0, dt0, p0, i0), (l1, dR1, dt1, p1, i1), (l2, dR2, dt2, p2, i2) = runs
    assert torch.equal(dR0, dR1) and torch.equal(dt0, dt1) and torch.equal(l0, l1) and torch.equal(i0, i1) and torch.equal(i0, i2)
    assert dR2 is None and dt2 is None and torch.equal(l0, l2)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
        assert torch.equal(p0[k], p2[k]), k                      # with / without requires_grad on the pose
    assert float(dR0.abs().max()) > 0 and float(dt0.abs().max()) > 0


def _finetune_stage(dev, sd_imu, sd_up, batch, use_graph):
    from mmego_amd import nets, nets_local
    from mmego_amd.train_step import StageStep
    himu = nets.IMUNet(15, 9, 512, 2, True, 0)
    himu.load_state_dict(sd_imu)
    himu = himu.to(dev).train()
    hup = nets_local.UpperNetwlocal()
    hup.load_state_dict(sd_up)
    hup = hup.to(dev).train()
    hup.lstm_dropout = 0
    st = StageStep("upper", hup, himu, lr=LR, use_graph=use_graph, finetune_imu=True, imu_lr=IMU_LR)
    x, imu, body, target = [v.to(dev) for v in batch]
    st.bind(x, imu, body, target)
    return st


DATA_SEED = 42          # (the issue's table of oracle-side margins between the 8th and 9th nearest point: 42, 43, 44, 45, 46 in this order)


def test_wlocal_finetune_step_against_oracle(dev):
    """test_finetune_step_against_oracle with UpperNetwlocal on both sides: B=4, T=8, N=128, IMU_Net(15, 9, 512, 2, True, 0) ->
    UpperNetwlocal without detach (oracle: fp32, CPU, one thread), nets seeded 41, data seeded DATA_SEED.  The two sides' poses differ by
    fp32 rounding, so the grouping precondition is asserted first.  Loss, prediction, every IMU_Net and every Upper gradient, the
    parameters after the two Adam steps (fc3, Q7, untouched); graph replay == eager bit for bit over two steps; no persistent-launch
    error."""
    from mmego_amd import blocks
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        B, T, N = 4, 8, 128
        torch.manual_seed(41)
        oimu = on.IMUNet(15, 9, 512, 2, True, 0).train()
        oup = on.UpperNetwlocal().train()
        set_lstm_dropout(oup, 0.0)
        sd_imu = {k: v.clone() for k, v in oimu.state_dict().items()}
        sd_up = {k: v.clone() for k, v in oup.state_dict().items()}
        g = torch.Generator().manual_seed(DATA_SEED)
        x = torch.randn(B, T, N, 6, generator=g)
        imu = torch.randn(B, T, 20, 15, generator=g)
        body = torch.randn(B, 20, 3, generator=g) * 0.3
        target = torch.randn(B, T, 21, 3, generator=g)
        batch = (x, imu, body, target)

        h0, c0 = ot.zeros_state(B)
        R, t = oimu(imu)                                             # (no torch.no_grad(), no .detach(): the fine-tuning body)
        lo = oup(x.clone(), h0, c0, h0, c0, body, R, t)[0]
        loss_o = ot.l1_sum(lo, target[:, :, list(sk.UPPER_MAP)])
        loss_o.backward()

        st = _finetune_stage(dev, sd_imu, sd_up, batch, use_graph=False)
        st.step()
        torch.cuda.synchronize()
        _same_groups(st.net.last_group_idx, oup.module2.last_group_idx, ("data seed", DATA_SEED))
        print("wlocal finetune step: loss %.6f / %.6f" % (st.loss.item(), loss_o.item()))
        assert abs(st.loss.item() - loss_o.item()) < 2e-5 * abs(loss_o.item()), (st.loss.item(), loss_o.item())
        assert torch.allclose(st.last_pred.cpu(), lo.detach(), rtol=1e-4, atol=2e-5), float((st.last_pred.cpu() - lo.detach()).abs().max())
        for tag, o, h in (("imu", oimu, st.imu), ("upper", oup, st.net)):
            po, ph = dict(o.named_parameters()), dict(h.named_parameters())
            flat = h.flat()
            scale = max(p.grad.abs().max().item() for p in po.values() if p.grad is not None)
            errs = {}
            for k in po:
                go = po[k].grad if po[k].grad is not None else torch.zeros_like(po[k])
                errs[k] = (flat.grad(ph[k]).detach().cpu() - go).abs().max().item()
            k_worst = max(errs, key=errs.get)
            print("wlocal finetune step: %s gradients, worst error %.3e (%s) at scale %.3e (%.2e of it)"
                  % (tag, errs[k_worst], k_worst, scale, errs[k_worst] / scale))
            for k, err in errs.items():
                assert err < GRAD_BAR * scale, (tag, k, err, scale)
        assert oimu.fc3.weight.grad is None

        # the two Adam steps
        torch.optim.Adam(oup.parameters(), lr=LR).step()
        torch.optim.Adam(oimu.parameters(), lr=IMU_LR, weight_decay=0.001).step()
        for tag, o, h, lr in (("imu", oimu, st.imu, IMU_LR), ("upper", oup, st.net, LR)):
            n_bad = n_all = 0
            sd_o, sd_h = o.state_dict(), h.state_dict()
            for k, p in o.named_parameters():
                if NOISE_GRAD.search(k):
                    continue
                dp = (sd_h[k].cpu() - sd_o[k]).abs()
                assert dp.max().item() <= 2 * lr + 2e-6, (tag, k, dp.max().item())
                n_bad += int((dp > 2e-6).sum())
                n_all += dp.numel()
            print("wlocal finetune step: %s parameters, %d of %d moved by more than 2e-6" % (tag, n_bad, n_all))
            assert n_bad < 0.05 * n_all, (tag, n_bad, n_all)
        for k in ("fc3.weight", "fc3.bias"):
            assert torch.equal(st.imu.state_dict()[k].cpu(), sd_imu[k]), k
        moved = [k for k, v in st.imu.state_dict().items() if not torch.equal(v.cpu(), sd_imu[k])]
        assert len(moved) == len(sd_imu) - 2, "every IMU_Net tensor but fc3 is trained"

        # graph replay == eager, bit for bit (two steps: the second replays the captured graph on updated weights)
        res = []
        for use_graph in (False, True):
            s2 = _finetune_stage(dev, sd_imu, sd_up, batch, use_graph=use_graph)
            losses = []
            for _ in range(2):
                losses.append(s2.step().item())
            torch.cuda.synchronize()
            assert (s2.graph is not None) == use_graph
            res.append((losses, s2.net.flat().flat_g.clone(), s2.net.flat().flat_p.clone(), s2.imu.flat().flat_g.clone(),
                        s2.imu.flat().flat_p.clone(), [b.clone() for b in s2.net.buffers()]))
        assert res[0][0] == res[1][0], (res[0][0], res[1][0])
        for a, b in zip(res[0][1:5], res[1][1:5]):
            assert torch.equal(a, b)
        for a, b in zip(res[0][5], res[1][5]):
            assert torch.equal(a, b)
        assert blocks.seq_xcd_errors() == 0
    finally:
        torch.set_num_threads(threads)


def _wlocal_stages(dev, imus, seed=91):
    """(Upper stage training an UpperNetwlocal, Lower stage behind a frozen UpperNetwlocal) on step_helpers' minibatch; ``imus``: "own"
    (each stage runs a frozen IMU_Net of its own) or "outside" (built with imu_net=None for an engine that supplies the pose; the two
    IMU_Nets are returned).  -> the stages, the IMU_Nets, the IMU samples and bind(), to call once the engine around the stages exists."""
    from mmego_amd import nets, nets_local
    from mmego_amd.train_step import StageStep
    x, imu_in, body, target, R = step_helpers.batch(dev)
    torch.manual_seed(seed)
    up = nets_local.UpperNetwlocal().to(dev).train()
    lo = nets.LowerNet(64).to(dev).train()
    fr = nets_local.UpperNetwlocal().to(dev).eval()
    imu_u, imu_l = nets.IMUNet(15, 9, 64, 2).to(dev).eval(), nets.IMUNet(15, 9, 64, 2).to(dev).eval()
    own = imus == "own"
    su = StageStep("upper", up, imu_u if own else None, lr=3e-5, use_graph=False)
    sl = StageStep("lower", lo, imu_l if own else None, upper_frozen=fr, lr=3e-5, use_graph=False)
    def bind():
        for st in (su, sl):
            st.bind(x.clone(), imu_in, body, target)
    return su, sl, (imu_u, imu_l), imu_in, bind


def _assert_same_stage(a, b, tag):
    assert a.loss.item() == b.loss.item(), (tag, a.stage, a.loss.item(), b.loss.item())
    assert torch.equal(a.net.flat().flat_g, b.net.flat().flat_g), (tag, a.stage)
    assert torch.equal(a.net.flat().flat_p, b.net.flat().flat_p), (tag, a.stage)
    for ba, bb in zip(a.net.buffers(), b.net.buffers()):
        assert torch.equal(ba, bb), (tag, a.stage)


def test_lower_stage_behind_a_frozen_wlocal_against_oracle(dev):
    """StageStep("lower", ..., upper_frozen=UpperNetwlocal in eval mode), recorded head pose, B=4, T=8, N=128, against the composition
    on.UpperNetwlocal eval forward -> .detach() -> on.LowerNet (train) on the once-transformed points, with the HIP step's top-64
    selection replayed (torch.sort's ties, as in the other Lower tests): loss, prediction and every Lower_Net gradient; the frozen net
    receives no gradient and keeps its buffers; graph replay == eager bit for bit over two steps."""
    from mmego_amd import nets, nets_local
    from mmego_amd.train_step import StageStep
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        B, T, N = 4, 8, 128
        torch.manual_seed(81)
        oup, olo = on.UpperNetwlocal().eval(), on.LowerNet(64).train()
        set_lstm_dropout(olo, 0.0)
        g = torch.Generator().manual_seed(82)
        for m in oup.modules():                                   # non-trivial running statistics
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)):
                m.running_mean.normal_(0.0, 0.2, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
        sd_up = {k: v.clone() for k, v in oup.state_dict().items()}
        sd_lo = {k: v.clone() for k, v in olo.state_dict().items()}
        x = torch.randn(B, T, N, 6, generator=g)
        body = torch.randn(B, 20, 3, generator=g) * 0.3
        target = torch.randn(B, T, 21, 3, generator=g)
        R = geo.rot6d_imu(torch.randn(B * T, 6, generator=g)).view(B, T, 3, 3).contiguous()

        def stage(use_graph):
            hup = nets_local.UpperNetwlocal()
            hup.load_state_dict(sd_up)
            hup = hup.to(dev).eval()
            hlo = nets.LowerNet(64)
            hlo.load_state_dict(sd_lo)
            hlo = hlo.to(dev).train()
            hlo.lstm_dropout = 0
            s = StageStep("lower", hlo, None, upper_frozen=hup, lr=LR, use_graph=use_graph)
            s.bind(x.to(dev), None, body.to(dev), target.to(dev), R_gt=R.to(dev))
            return s
        st = stage(False)
        st._body()
        torch.cuda.synchronize()
        idx = st.net.last_select_idx.clone().cpu()

        h0, c0 = ot.zeros_state(B)
        t = target[:, :, 20].contiguous()
        x1 = x.clone()
        with torch.no_grad():
            up_o = oup(x1, h0, c0, h0, c0, body, R, t)[0]
        _same_groups(st.upper_frozen.last_group_idx, oup.module2.last_group_idx, "frozen wlocal")
        lo_o = olo(up_o.detach(), x1.detach().clone(), None, None, None, None, body, R, t, pin_select_idx=idx)[0]
        loss_o = ot.l1_sum(lo_o, target[:, :, list(sk.LOWER_MAP)])
        loss_o.backward()
        print("lower behind wlocal: loss %.6f / %.6f" % (st.loss.item(), loss_o.item()))
        assert abs(st.loss.item() - loss_o.item()) < 2e-5 * abs(loss_o.item()), (st.loss.item(), loss_o.item())
        assert torch.allclose(st.last_pred.cpu(), lo_o.detach(), rtol=1e-4, atol=2e-5), float((st.last_pred.cpu() - lo_o.detach()).abs().max())
        po, ph = dict(olo.named_parameters()), dict(st.net.named_parameters())
        flat = st.net.flat()
        scale = max(p.grad.abs().max().item() for p in po.values() if p.grad is not None)
        worst = 0.0
        for k in po:
            go = po[k].grad if po[k].grad is not None else torch.zeros_like(po[k])
            err = (flat.grad(ph[k]).detach().cpu() - go).abs().max().item()
            worst = max(worst, err)
            assert err < GRAD_BAR * scale, (k, err, scale)
        print("lower behind wlocal: gradients, worst error %.3e at scale %.3e (%.2e of it)" % (worst, scale, worst / scale))
        for k, v in st.upper_frozen.state_dict().items():          # frozen: eval mode, nothing written
            assert torch.equal(v.cpu(), sd_up[k]), k
        assert st.upper_opt is None and st.imu_opt is None

        res = []
        for use_graph in (False, True):
            s2 = stage(use_graph)
            losses = [s2.step().item() for _ in range(2)]
            torch.cuda.synchronize()
            assert (s2.graph is not None) == use_graph
            res.append((losses, s2.net.flat().flat_g.clone(), s2.net.flat().flat_p.clone(), [b.clone() for b in s2.net.buffers()]))
        assert res[0][0] == res[1][0], (res[0][0], res[1][0])
        assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
        for a, b in zip(res[0][3], res[1][3]):
            assert torch.equal(a, b)
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("kind", ["concurrent", "pipelined", "shared"])
def test_step_engines_around_wlocal_stages_equal_plain_steps(dev, kind):
    """ConcurrentStages, PipelinedStages and SharedImuStages around an Upper stage that trains an UpperNetwlocal and a Lower stage behind a
    frozen one, as HIP graphs: losses, gradients, parameters and BatchNorm buffers of both stages equal the plain StageSteps', run one after
    the other, bit for bit over two steps."""
    from mmego_amd import blocks
    from mmego_amd.train_step import ConcurrentStages, PipelinedStages, SharedImuStages
    ref_u, ref_l, _, _, bind = _wlocal_stages(dev, "own")
    if kind == "shared":                                          # (one IMU_Net for both stages: the reference stages run the same one)
        ref_l.imu = ref_u.imu
    bind()
    for _ in range(2):
        ref_u.step()
        ref_l.step()
    if kind == "concurrent":
        su, sl, _, _, bind = _wlocal_stages(dev, "own")
        eng = ConcurrentStages([su, sl], use_graph=True)
        bind()
    elif kind == "pipelined":
        su, sl, imus, imu_in, bind = _wlocal_stages(dev, "outside")
        eng = PipelinedStages([su, sl], list(imus), imu_in, use_graph=True)
        bind()
        eng.prime()
    else:
        su, sl, imus, imu_in, bind = _wlocal_stages(dev, "outside")
        eng = SharedImuStages(imus[0], [su, sl], imu_in, use_graph=True)
        bind()
    for _ in range(2):
        eng.step()
    torch.cuda.synchronize()
    assert eng.graph is not None
    _assert_same_stage(su, ref_u, kind)
    _assert_same_stage(sl, ref_l, kind)
    assert blocks.seq_xcd_errors() == 0


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
RESULT_LINES = ("Average Joint Localization Error(cm):", "Average UpperBody Joint Localization Error(cm):",
                "Average LowerBody Joint Localization Error(cm):", "Average Joint Rotation Error", "Per Joint Localization Error(cm):")


def _checkpoints(mdir):
    return [f for f in glob.glob(os.path.join(mdir, "epoch*_batch4frame*.pth")) if not f.endswith(".train_state.pth")]


def test_cli_upper_variant_wlocal_train_resume_lower_infer(tmp_path):
    """--upper_variant wlocal through the command line, one epoch each at --batch_size 4, recorded head pose: stage 2 writes a checkpoint
    that loads into UpperNetwlocal (and not into UpperNet); --resume continues from it; stage 3 and --infer load it as their Upper_Net and
    print what they print for the global variant; a global checkpoint under the flag ends with the message that names it."""
    from test_cli_gpu import _make_dataset, _run
    from mmego_amd import nets, nets_local
    data = str(tmp_path / "Sample_data")
    _make_dataset(data, np.random.default_rng(4))
    out_dir = str(tmp_path / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    common = ["--gt_head_pose", "--data_root", data, "--batch_size", "4", "--device", "cuda:0", "--seed", "0", "--upper_variant", "wlocal"]
    out = _run(["--train", "--network", "Upper_Net", "--epochs", "1", "--log_dir", "9301"] + common, env)
    assert "epoch: 1" in out and "Average Joint Localization Error" in out
    first = _checkpoints(os.path.join(out_dir, "model", "9301"))
    assert len(first) == 1 and os.path.exists(first[0][:-4] + ".train_state.pth")
    sd = torch.load(first[0], map_location="cpu")
    nets_local.UpperNetwlocal().load_state_dict(sd)
    assert any(k.startswith("module2.") for k in sd) and not any(k.startswith("mlpHead.") for k in sd)
    assert all(bool(torch.isfinite(v.float()).all()) for v in sd.values())
    # --resume
    out = _run(["--train", "--network", "Upper_Net", "--epochs", "2", "--log_dir", "9302", "--resume", first[0]] + common, env)
    assert "resumed from" in out and "epoch: 2" in out and "epoch: 1\n" not in out
    second = _checkpoints(os.path.join(out_dir, "model", "9302"))
    assert len(second) == 1 and os.path.basename(second[0]).startswith("epoch1_")
    sd2 = torch.load(second[0], map_location="cpu")
    assert sd2.keys() == sd.keys() and any(not torch.equal(sd2[k], sd[k]) for k in sd)
    # stage 3 behind it, and --infer
    torch.manual_seed(0)
    lower_ck = str(tmp_path / "lower.pth")
    torch.save(nets.LowerNet(64).state_dict(), lower_ck)
    out = _run(["--train", "--network", "Lower_Net", "--epochs", "1", "--log_dir", "9303", "--load_Upper_path", first[0]] + common, env)
    assert "epoch: 1" in out and "Average LowerBody Joint Localization Error" in out
    assert len(_checkpoints(os.path.join(out_dir, "model", "9303"))) == 1
    assert not os.path.exists(os.path.join(out_dir, "model", "9303", "Upper_Net"))       # frozen: nothing saved for it
    out = _run(["--infer", "--gt_head_pose", "--data_root", data, "--device", "cuda:0", "--upper_variant", "wlocal", "--load_Upper_path", first[0],
                "--load_Lower_path", lower_ck], env)
    for line in RESULT_LINES:
        assert line in out, line
    # a checkpoint of the other variant
    global_ck = str(tmp_path / "upper_global.pth")
    torch.save(nets.UpperNet().state_dict(), global_ck)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--infer", "--gt_head_pose", "--data_root", data, "--device", "cuda:0",
                        "--upper_variant", "wlocal", "--load_Upper_path", global_ck, "--load_Lower_path", lower_ck],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "--upper_variant global" in r.stderr and "Missing key" not in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]


def test_cli_upper_variant_wlocal_finetune_imu(tmp_path):
    """--train --network Upper_Net --upper_variant wlocal --finetune_imu: the IMU_Net checkpoint is saved beside the Upper one, its weights
    moved (fc3, never trained, as it was), the Upper checkpoint an UpperNetwlocal's."""
    from test_cli_gpu import _make_dataset, _run
    from mmego_amd import nets, nets_local
    data = str(tmp_path / "Sample_data")
    _make_dataset(data, np.random.default_rng(5))
    torch.manual_seed(2)
    imu_ck = str(tmp_path / "imu.pth")
    start = nets.IMUNet(15, 9, 512, 2, True, 0.1).state_dict()
    torch.save(start, imu_ck)
    start = {k: v.clone() for k, v in start.items()}
    out_dir = str(tmp_path / "train_out")
    env = dict(os.environ, PYTHONPATH=ROOT, MMEGO_TRAIN_DIR=out_dir)
    out = _run(["--train", "--network", "Upper_Net", "--upper_variant", "wlocal", "--finetune_imu", "--imu_lr", "1e-4", "--load_IMU_path", imu_ck,
                "--data_root", data, "--epochs", "1", "--batch_size", "4", "--device", "cuda:0", "--seed", "0", "--log_dir", "9311"], env)
    assert "epoch: 1" in out and "Average Joint Localization Error" in out
    mdir = os.path.join(out_dir, "model", "9311")
    up = _checkpoints(mdir)
    im = glob.glob(os.path.join(mdir, "IMU_Net", "epoch0_batch4frame*.pth"))
    assert len(up) == 1 and len(im) == 1, os.listdir(mdir)
    assert os.path.basename(up[0]) == os.path.basename(im[0])
    nets_local.UpperNetwlocal().load_state_dict(torch.load(up[0], map_location="cpu"))
    got = torch.load(im[0], map_location="cpu")
    nets.IMUNet(15, 9, 512, 2, True, 0).load_state_dict(got)
    for k in start:
        assert bool(torch.isfinite(got[k]).all()), k
        if k.startswith("fc3."):
            assert torch.equal(got[k], start[k]), k
        else:
            assert not torch.equal(got[k], start[k]), k
    log = open(os.path.join(out_dir, "report", "9311", "log-loss.txt")).read().split()
    assert np.isfinite(float(log[1]))
