"""CPU: the float64 references and bounds of tests/lstm_ref.py, before any GPU sees them.

  * the sequence reference, forward and backward, IS torch.nn.LSTM(bidirectional=True) in float64 and its autograd (1e-12);
  * an fp32 emulation of every kernel's arithmetic stays inside every bound WITHOUT the margin (ratio <= 1) at every shape and input
    distribution of tests/test_lstm_kernels_gpu.py, the saturated and the near-zero rows included;
  * host-side mirrors of mmego_lstm_step's and lstm_bwd_step_dma_try's kernel choice, held to the sources, pin that the GPU file's cases
    reach every kernel and template instantiation they claim to."""
import os
import re

import pytest
import torch

import lstm_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmego_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------------------------
# agreement with torch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", (32, 64))
@pytest.mark.parametrize("state", (True, False))
def test_sequence_reference_is_torch_lstm(H, state):
    """Forward and backward.  The LSTM's input is [xproj_0, xproj_1] (8H wide) and W_ih of direction d selects its half with b_ih = 0, so
    the gradient with respect to the input IS the gradient with respect to the pre-activations of both directions."""
    B, T = 5, 4
    g = torch.Generator().manual_seed(100 + H + int(state))
    lstm = torch.nn.LSTM(8 * H, H, bidirectional=True, batch_first=True).double()
    W, b = [], []
    with torch.no_grad():
        for d, sfx in enumerate(("", "_reverse")):
            wih = torch.zeros(4 * H, 8 * H, dtype=torch.float64)
            wih[:, d * 4 * H:(d + 1) * 4 * H] = torch.eye(4 * H, dtype=torch.float64)
            getattr(lstm, "weight_ih_l0" + sfx).copy_(wih)
            getattr(lstm, "bias_ih_l0" + sfx).zero_()
            W.append(getattr(lstm, "weight_hh_l0" + sfx).detach().clone())
            b.append(getattr(lstm, "bias_hh_l0" + sfx).detach().clone())
    x = torch.randn(B, T, 8 * H, generator=g, dtype=torch.float64).requires_grad_(True)
    h0 = torch.randn(2, B, H, generator=g, dtype=torch.float64) * 0.5
    c0 = torch.randn(2, B, H, generator=g, dtype=torch.float64) * 0.5
    out, (hn, cn) = lstm(x, (h0, c0)) if state else lstm(x)
    dout = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64)
    out.backward(dout)
    xp = [x.detach()[:, :, :4 * H], x.detach()[:, :, 4 * H:]]
    st = [h0[0], h0[1]] if state else [None, None]
    ct = [c0[0], c0[1]] if state else [None, None]
    ref = R.seq_fwd(xp, W, b, st, ct)
    assert (ref["out"][0] - out.detach()).abs().max() < 1e-12
    for d in range(2):
        assert (ref["hn"][d][0] - hn[d].detach()).abs().max() < 1e-12 and (ref["cn"][d][0] - cn[d].detach()).abs().max() < 1e-12
    back = R.seq_bwd(dout, ref["gates"], ref["cst"], ct, W)
    for d in range(2):
        assert (back[d][0] - x.grad[:, :, d * 4 * H:(d + 1) * 4 * H]).abs().max() < 1e-12, d


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation stays inside the bounds (no MARGIN)
# ---------------------------------------------------------------------------------------------------------------------------------
def inside(what, out, ref, bound):
    r, idx = R.worst_ratio(out, ref, bound)
    assert r <= 1.0, "%s: emulation / bound ratio %.3g at %s" % (what, r, idx)
    return r


def test_activation_bounds_hold_for_the_emulation():
    """Dense sweeps, the saturated ends and tanh's absolute-error regime; and the claim the header used to make is false: near zero the
    fast tanh is nowhere near a few ulp of tanh."""
    g = torch.Generator().manual_seed(5)
    for lo in (1e-6, 1e-3, 1.0, 20.0, 100.0):
        x = (torch.rand(200000, generator=g) * 2 - 1) * lo
        inside("sigmoid", R.emu_sigmoid(x), *R.sigmoid(x.double()))
        inside("tanh", R.emu_tanh(x), *R.tanh_fast(x.double()))
    x = (torch.rand(200000, generator=g) * 2 - 1) * 1e-3
    rel = ((R.emu_tanh(x).double() - torch.tanh(x.double())).abs() / torch.tanh(x.double()).abs()).max()
    assert rel > 1e-3            # (about 1e-2 and beyond: a relative claim cannot hold there)
    # exact saturation: 1 - g and 1 - tc^2 are exactly 0 in the backward
    assert R.emu_sigmoid(torch.tensor([20.0, 100.0, -100.0])).tolist() == [1.0, 1.0, 0.0]
    assert R.emu_tanh(torch.tensor([20.0, -20.0, 100.0, -100.0])).tolist() == [1.0, -1.0, 1.0, -1.0]


@pytest.mark.parametrize("B", R.L64_B)
@pytest.mark.parametrize("T", R.L64_T)
def test_emulated_lstm64_inside_bounds(B, T):
    for shift in ((0, 1, 2) if B == 1 else (0,)):
        o = R.l64_opts(B, T, shift)
        for c0key in ("c0", "bc0"):          # the forward's options, and the forward that writes the backward test's stashes
            I = R.seq_inputs(B, T, shift, with_b=o["bhh"])
            b = I["b"]
            h0 = [I["h0"][d] if o["h0"][d] else None for d in range(2)]
            c0 = [I["c0"][d] if o[c0key][d] else None for d in range(2)]
            emu = R.emu_seq_fwd(I["xp"], I["W"], b, h0, c0)
            ref = R.seq_fwd(I["xp"], I["W"], b, h0, c0)
            inside("chain out", emu["out"], *ref["out"])
            for d in range(2):
                inside("chain hn", emu["hn"][d], *ref["hn"][d])
                inside("chain cn", emu["cn"][d], *ref["cn"][d])
                for s in range(T):      # step by step from the emulation's own state
                    t = s if d == 0 else T - 1 - s
                    cp = (emu["cst"][d][t - 1 if d == 0 else t + 1] if s > 0 else (torch.zeros(B, 64) if c0[d] is None else c0[d]))
                    st = R.step(I["xp"][d][:, t], b[d], emu["hprev"][d][:, t], I["W"][d], cp, "lstm64")
                    inside("step gates", emu["gates"][d][t].permute(0, 2, 1).reshape(B, 256), *st["gates"])
                    inside("step c", emu["cst"][d][t], *st["c"])
                    inside("step h", emu["out"][:, t, d * 64:(d + 1) * 64], *st["h"])
            back = R.seq_bwd(I["dout"], emu["gates"], emu["cst"], c0, I["W"], "fast")
            eb = R.emu_seq_bwd(I["dout"], emu["gates"], emu["cst"], c0, I["W"])
            for d in range(2):
                inside("chain dgates", eb[d], *back[d])


def step_cases(ncu=256):
    return R.STEP_CASES + [(2, R.smallest_dma32_bn(2, 512, ncu), 512, 0, 0, "lstm_step_dma_kernel<32>")]


KIND = {"lstm_first_step_kernel": "first", "lstm_step_dma_kernel": "dma", "lstm_step_small_kernel": "small"}


@pytest.mark.parametrize("case", step_cases(), ids=lambda c: "-".join(str(v) for v in c[:5]))
def test_emulated_step_inside_bounds(case):
    ndir, Bn, H, first, _, kernel = case
    I = R.step_inputs(ndir, Bn, H)
    kind = "first" if first else KIND[kernel.split("<")[0]]
    for d in range(ndir):
        hp, cp = (torch.zeros(Bn, H), torch.zeros(Bn, H)) if first else (I["h"][d], I["c"][d])
        emu = R.emu_step(I["xp"][d], I["b"][d], hp, I["W"][d], cp, "first" if first else kind)
        # (the first step through a general kernel forms f * 0 + i g: the same value as the first-step kernel's i g)
        ref = R.step(I["xp"][d], I["b"][d], hp, I["W"][d], cp, kind)
        for k in ("gates", "c", "h"):
            inside(k, emu[k], *ref[k])


@pytest.mark.parametrize("case", R.CELL_BWD_CASES + [(2, c[0], c[1]) for c in R.BWD_STEP_CASES], ids=str)
def test_emulated_cell_backward_inside_bounds(case):
    ndir, Bn, H = case
    I = R.bwd_inputs(ndir, Bn, H)
    for d in range(ndir):
        gs = I["gst"][d]
        gates = (gs[:, :H], gs[:, H:2 * H], gs[:, 2 * H:3 * H], gs[:, 3 * H:])
        for rec in (False, True):
            for cp in (None, I["cprev"][d]):
                dh = I["dout"][d] + I["dhrec"][d] if rec else I["dout"][d]
                ref = R.cell_bwd(*gates, I["cst"][d], cp, I["dc"][d], I["dout"][d].double() + (I["dhrec"][d].double() if rec else 0.0),
                                 0.0, R.U32 * dh.double().abs() if rec else 0.0, "libm")
                emu = R.emu_cell_bwd(*gates, torch.tanh(I["cst"][d]), torch.zeros(Bn, H) if cp is None else cp, I["dc"][d], dh)
                for k in emu:
                    inside(k, emu[k], *ref[k])
        # the recurrent form: dh = dout + dgn . W in fp32
        ref = R.bwd_step(I["dgn"][d], I["W"][d], I["dout"][d], gs, I["cst"][d], I["cprev"][d], I["dc"][d], 2)
        emu = R.emu_cell_bwd(*gates, torch.tanh(I["cst"][d]), I["cprev"][d], I["dc"][d], I["dout"][d] + I["dgn"][d] @ I["W"][d])
        for k in emu:
            inside("bwd_step " + k, emu[k], *ref[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# dispatch mirrors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_step_dispatch_table_reaches_every_kernel():
    """Every kernel and instantiation of csrc/lstm_step.hip is reached by a case of the GPU file, on a whole MI355X (256 CUs) and on a
    partition of it (the <32> case is computed from the CU count); the LDS-DMA kernel at 1, 2, 3, 4 and 16 chunks, with and without the
    XCD order; the first step through each general kernel family."""
    reached = set()
    for ndir, Bn, H, first, boff, want in step_cases(256):
        got = R.step_kernel(bool(first), not boff, ndir, Bn, H, 256)
        assert got == want, (ndir, Bn, H, first, boff, got, want)
        reached.add(want)
    assert reached == {"lstm_first_step_kernel", "lstm_step_small_kernel<64, true, 8>", "lstm_step_small_kernel<64, true>",
                       "lstm_step_small_kernel<64, false>", "lstm_step_small_kernel<32, true>", "lstm_step_small_kernel<32, false>",
                       "lstm_step_dma_kernel<16>", "lstm_step_dma_kernel<32>"}
    for ncu in (304, 256, 128, 64):
        bn = R.smallest_dma32_bn(2, 512, ncu)
        assert bn % 64 == 8 and R.step_kernel(False, True, 2, bn, 512, ncu) == "lstm_step_dma_kernel<32>"
        assert bn - 64 < 128 or R.step_kernel(False, True, 2, bn - 64, 512, ncu) == "lstm_step_dma_kernel<16>"
    assert R.smallest_dma32_bn(2, 512, 256) == 264       # 2 * grid32 = 2 * 2 * 16 * 5 = 320 > 256; at four row blocks it is 256 <= 256
    dma16 = [c for c in R.STEP_CASES if c[5] == "lstm_step_dma_kernel<16>"]
    assert {R.step_dma(c[3], c[0], c[1], c[2], 16)[0] for c in dma16} == {0, 1, 2, 3, 4}
    assert {(c[2], R.step_dma(c[3], c[0], c[1], c[2], 16)[2]) for c in dma16 if not c[3]} == {(32, False), (64, True), (96, False), (128, True)}
    assert {c[1] for c in dma16} == {128, 136}
    for nk, first in ((0, 1), (1, 0), (2, 0), (3, 0), (4, 0), (16, 0)):
        assert R.step_dma(first, 2, 128, 32 * max(nk, 1), 16)[1] == (2 if first else nk + 1)
    # first step through the general kernels: b_hh off alignment
    assert {c[5].split("<")[0] for c in R.STEP_CASES if c[3] and c[4]} == {"lstm_step_small_kernel", "lstm_step_dma_kernel"}


def test_step_dispatch_mirror_matches_the_source():
    """The conditions the mirror restates are the ones in the launcher (a changed threshold fails here, not silently in the table)."""
    src = open(os.path.join(CSRC, "lstm_step.hip")).read()
    for needle in ("if (first && (H % 4) == 0 && (al & 15) == 0)", "} else if (Bn >= 128) {", "const int grid32 = ndir * (H / 32) * cdiv(Bn, 64);",
                   "const bool ht16 = 2 * grid32 <= (ncu > 0 ? ncu : 256);", "const bool full = (Bn % 64) == 0;", "if (H == 512 && full) {",
                   "else if ((H % 64) == 0) { if (full) SMALL_LAUNCH(64, true); else SMALL_LAUNCH(64, false); }",
                   "else { if (full) SMALL_LAUNCH(32, true); else SMALL_LAUNCH(32, false); }", "const int nk = first ? 0 : H / 32;",
                   "const int id = (npairs & 7) == 0 ? xcd_order(blockIdx.x, npairs * nrb) : (int)blockIdx.x;"):
        assert needle in src, needle
    al = re.search(r"const uintptr_t al = ([^;]*);", src).group(1)
    assert sorted(re.findall(r"\(uintptr_t\)(\w+)", al)) == sorted(["bhh0", "bhh1", "gst0", "gst1", "cst0", "cst1", "c1", "hout1", "xproj1"])
    src = open(os.path.join(CSRC, "lstm_bwd_step.hip")).read()
    assert "if (!on || Bn % 64 != 0 || H % 32 != 0 || (dgs & 3) != 0) return -1;" in src and "const int on = env ? atoi(env) : 1;" in src


def test_bwd_step_dispatch_table():
    reached = {}
    for Bn, H, env, want in R.BWD_STEP_CASES:
        assert R.bwd_step_kernel(env, Bn, H, 2 * 8 * H) == want, (Bn, H, env)
        reached.setdefault(want, set()).add((Bn, 4 * H // 64))
    assert {k for _, k in reached["lstm_bwd_step_dma_kernel"]} == {2, 4, 6, 8, 32}       # K = 4H in 64-k chunks
    assert {b for b, _ in reached["gemm32kq_kernel<true, true>"]} == {32, 96, 64}
    assert R.bwd_step_kernel(None, 64, 64, 1024, aligned=False).startswith("gemm32kq") and R.bwd_step_kernel("1", 64, 64, 1024) == "lstm_bwd_step_dma_kernel"


def test_lstm64_cases_reach_all_eight_instantiations():
    got = {R.l64_inst(B, s, d) for B in R.L64_B for s in (0, 1) for d in (0, 1)}
    assert len(got) == 8 and {B % 16 == 0 for B in R.L64_B} == {True, False}
    assert {(B // 16, B % 16 != 0) for B in R.L64_B} == {(0, True), (1, False), (1, True), (2, True)}   # ragged alone, full, full + ragged


# ---------------------------------------------------------------------------------------------------------------------------------
# stage-1 loss and 6-D head
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", R.IMU_F)
def test_imu_loss_reference_and_emulation(F):
    """The restated loss and gradients are float64 autograd's; clamped frames and t == head frames have exactly zero gradients; the fp32
    emulation stays inside the bounds."""
    inp = R.imu_loss_inputs(F)
    (loss, e_loss), (dR, e_dR), (dt, e_dt) = R.imu_loss(*inp, 0.25)
    l2, dR2, dt2 = R.imu_loss_autograd(*inp, 0.25)
    assert abs(loss - l2) < 1e-9 * abs(l2) and (dR - dR2).abs().max() < 1e-9 * dR2.abs().max().clamp_min(1) and (dt - dt2).abs().max() < 1e-9
    for f in range(F):
        if f % 4 == 1:
            assert bool((dR[f] == 0).all())
        if f % 4 == 2:
            assert bool((dt[f] == 0).all())
    el, edR, edt = R.emu_imu_loss(*inp, 0.25)
    inside("loss", el, loss, e_loss)
    inside("dR", edR, dR, e_dR)
    inside("dt", edt, dt, e_dt)


@pytest.mark.parametrize("F", R.IMU_F)
def test_imu_head_reference_and_emulation(F):
    y, dR, dt = R.imu_head_inputs(F)
    (Rr, eR), (tr, et) = R.imu_head(y)
    eR_, et_ = R.emu_imu_head(y)
    inside("R", eR_, Rr, eR)
    inside("t", et_, tr, et)
    ref, e = R.imu_head_bwd(y, dR, dt)
    inside("dy", R.emu_imu_head_bwd(y, dR, dt), ref, e)
    if F > 2:
        assert bool((Rr[1] == 0).all()) and bool((Rr[2].view(3, 3)[:, 1:] == 0).all())       # the eps branches: zero columns


# ---------------------------------------------------------------------------------------------------------------------------------
# the bounds are tight enough to catch a wrong kernel: five mutants of the EMULATION, one per kernel family
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mutated_emulations_are_far_outside_the_bounds():
    """Each mutant changes arithmetic or a selection among in-bounds elements, as a subtly wrong kernel would; each must push a ratio
    far past MARGIN (> 100) in the comparison named.  (Run on the emulation: a kernel made wrong on purpose never runs on a GPU.)"""
    far = {}
    B, T = 17, 5
    I = R.seq_inputs(B, T)
    emu = R.emu_seq_fwd(I["xp"], I["W"], I["b"], I["h0"], I["c0"])
    # 1. lstm64 forward: two gates swapped in the stash store (f <-> g)
    st = R.step(I["xp"][0][:, 0], I["b"][0], emu["hprev"][0][:, 0], I["W"][0], I["c0"][0], "lstm64")
    sw = emu["gates"][0][0][:, :, [0, 2, 1, 3]]
    far["lstm64_fwd stash gates"] = R.worst_ratio(sw.permute(0, 2, 1).reshape(B, 256), *st["gates"])[0]
    # 2. lstm64 backward: direction 1's c_{t-1} taken from the wrong neighbour (t - 1 instead of t + 1)
    back = R.seq_bwd(I["dout"], emu["gates"], emu["cst"], I["c0"], I["W"], "fast")
    dg, dc, rec = torch.zeros(B, T, 256), torch.zeros(B, 64), torch.zeros(B, 64)
    for s in range(T - 1, -1, -1):
        t = T - 1 - s
        cprev = emu["cst"][1][max(t - 1, 0)] if s > 0 else I["c0"][1]
        G = emu["gates"][1][t]
        r = R.emu_cell_bwd(G[:, :, 0], G[:, :, 1], G[:, :, 2], G[:, :, 3], R.emu_tanh(emu["cst"][1][t]), cprev, dc, I["dout"][:, t, 64:] + rec)
        dg[:, t] = torch.cat([r[k] for k in ("di", "df", "dg", "do")], -1)
        dc, rec = r["dcprev"], dg[:, t] @ I["W"][1]
    far["lstm64_bwd dgates1"] = R.worst_ratio(dg, *back[1])[0]
    # 3. lstm_step_small: the o gate fetched from the g gate's lane
    J = R.step_inputs(1, 37, 96)
    e = R.emu_step(J["xp"][0], J["b"][0], J["h"][0], J["W"][0], J["c"][0], "small")
    ref = R.step(J["xp"][0], J["b"][0], J["h"][0], J["W"][0], J["c"][0], "small")
    far["small h"] = R.worst_ratio(e["gates"][:, 192:288] * R.emu_tanh(e["c"]), *ref["h"])[0]
    # 4. cell backward: 1 - tc * tc written as 1 - tc;  5. dcprev written as dcv * gi
    K = R.bwd_inputs(1, 37, 32)
    gs, H = K["gst"][0], 32
    gates = (gs[:, :H], gs[:, H:2 * H], gs[:, 2 * H:3 * H], gs[:, 3 * H:])
    ref = R.cell_bwd(*gates, K["cst"][0], K["cprev"][0], K["dc"][0], K["dout"][0].double(), 0.0, 0.0, "libm")
    tc = torch.tanh(K["cst"][0])
    dcv4 = K["dc"][0] + K["dout"][0] * gates[3] * (1.0 - tc)
    far["cell_bwd dgates"] = R.worst_ratio(dcv4 * gates[2] * gates[0] * (1.0 - gates[0]), *ref["di"])[0]
    dcv = K["dc"][0] + K["dout"][0] * gates[3] * (1.0 - tc * tc)
    far["cell_bwd dc"] = R.worst_ratio(dcv * gates[0], *ref["dcprev"])[0]
    print("\n".join("MUTANT %-24s ratio %.3g" % kv for kv in far.items()))
    assert all(v > 100.0 for v in far.values()), far
