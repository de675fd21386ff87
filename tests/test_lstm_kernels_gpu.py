"""GPU: the LSTM recurrence kernels, each on its own through the C ABI, against float64 (tests/lstm_ref.py): the H = 64 whole-sequence pair
of csrc/lstm.hip and its _multi forms, the three step kernels of csrc/lstm_step.hip, the backward step of csrc/lstm_bwd_step.hip and its
K-quartered form in csrc/gemm.hip, the pointwise cell backward and the stage-1 loss of csrc/imu_train.hip.

Method of tests/test_gcn_train_gpu.py (its helpers are used where they fit): every reference is plain float64 torch on the CPU computed
from the fp32 values the kernel read; |out - ref| <= MARGIN * bound elementwise with the a-priori bounds lstm_ref.py derives (MARGIN = 4);
no element is left out of any comparison; strided operands lie in wider buffers with NaN around them (the other direction's columns of the
production layouts); every output is surrounded by a sentinel that must survive (guard rows, guard columns, the unused half of a 256-wide
out).  Recurrences with a stash are checked step by step from the kernel's OWN fp32 h_{t-1} / c_{t-1} (no amplification), the others
against a chain that carries a first-order bound beside each value.  Every case has ordinary rows (pre-activations of order 1, weights at
nn.LSTM's initialisation scale), saturated rows (pre-activations +-20 and +-100: gates exactly 0 / 1, exp inf or 0) and near-zero rows
(pre-activations and c below 1e-3: fast_tanh's absolute-error regime).  NOTES.md ("Float64 tests of the LSTM recurrence kernels") holds the
measured error / bound ratios; tests/test_lstm_ref_cpu.py pins which kernel each case reaches."""
import pytest
import torch

import lstm_ref as R
from lstm_ref import MARGIN
from test_gcn_train_gpu import Out, d_vec, refused, call, SENT, GUARD, NAN

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mmego_amd import hip
    hip.lib()
    yield torch.device("cuda:0")
    if RATIOS:
        print("\nlargest |out - ref| / bound per kernel and output (bound without MARGIN):")
        for (k, o), r in sorted(RATIOS.items()):
            print("RATIO %-24s %-14s %.4g" % (k, o, r))


def check(kernel, name, out, ref, bound, note=""):
    """|out - ref| <= MARGIN * bound elementwise, every element; records the largest error / bound ratio."""
    worst, idx = R.worst_ratio(out.cpu(), ref, bound)
    RATIOS[(kernel, name)] = max(RATIOS.get((kernel, name), 0.0), worst)
    if not worst <= MARGIN:
        o, b = out.cpu().double(), torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
        raise AssertionError("%s %s %s: worst at %s: got %r want %r bound %.3g (ratio %.3g)"
                             % (kernel, name, note, idx, float(o[idx]), float(ref[idx]), float(b[idx]), worst))


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Wide:
    """A [rows][C] window at column `col` of a [rows + guard][ld] buffer filled with `fill` -- NaN around an operand, the sentinel around
    an output -- with `lead` floats in front of it (lead = 1: a base 4 bytes past an aligned address)."""

    def __init__(self, dev, rows, C, ld, col=0, fill=SENT, src=None, lead=0, guard=GUARD):
        self.rows, self.C, self.ld, self.col, self.fill, self.lead, self.guard = rows, C, ld, col, fill, lead, guard
        self.buf = torch.full((lead + (rows + guard) * ld,), fill, dtype=torch.float32, device=dev)
        self.view = self.buf[lead:].view(rows + guard, ld)[:rows, col:col + C]
        if src is not None:
            self.view.copy_(src.reshape(rows, C))

    def cpu(self):
        return self.view.cpu()

    def guards_intact(self):
        b = self.buf.clone()
        b[self.lead:].view(self.rows + self.guard, self.ld)[:self.rows, self.col:self.col + self.C] = self.fill
        return bool(torch.isnan(b).all()) if self.fill != self.fill else bool((b == self.fill).all())


def dense(dev, t):
    """An in / out state [rows][C] with sentinel guard rows behind it."""
    rows, C = t.shape
    return Wide(dev, rows, C, C, src=t)


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_lstm64_forward / _backward
# ---------------------------------------------------------------------------------------------------------------------------------
OPTS = R.L64_OPTS
DROP_P = 0.25


class L64:
    """One mmego_lstm64_forward call: device buffers, the argument list, the descriptor of the _multi form."""

    def __init__(self, dev, I, B, T, o, stash, drop, salt=3):
        self.B, self.T, self.I, self.o, self.stash, self.drop = B, T, I, o, stash, drop
        xs = o["xs"]
        self.xp = Wide(dev, B * T, 512, xs, fill=NAN, src=torch.cat((I["xp"][0], I["xp"][1]), -1))     # both directions in one buffer
        self.W = [d_vec(dev, w) for w in I["W"]]
        self.b = [None if b is None else d_vec(dev, b) for b in I["b"]]
        self.h0 = [d_vec(dev, I["h0"][d]) if o["h0"][d] else None for d in range(2)]
        self.c0 = [d_vec(dev, I["c0"][d]) if o["c0"][d] else None for d in range(2)]
        self.out = Wide(dev, B * T, 128, o["os"])
        self.hn = [Out(dev, B, 64, strided=False) for _ in range(2)]
        self.cn = [Out(dev, B, 64, strided=False) for _ in range(2)]
        self.gates = [Wide(dev, T * B, 256, 256) if stash else None for _ in range(2)]
        self.cst = [Wide(dev, T * B, 64, 64) if stash else None for _ in range(2)]
        self.hprev = [Wide(dev, B * T, 64, 64) if stash else None for _ in range(2)]
        self.dy = Wide(dev, B * T, 128, o["os"]) if drop else None
        self.dm = Wide(dev, B * T, 128, o["os"]) if drop else None
        self.seed = torch.tensor([12345], dtype=torch.int64, device=dev) if drop else None
        self.salt = salt
        v = lambda w: None if w is None else w.view
        self.args = [B, T, self.xp.view, self.xp.view[:, 256:], xs, self.W[0], self.W[1], self.b[0], self.b[1], self.h0[0], self.h0[1],
                     self.c0[0], self.c0[1], self.out.view, o["os"], self.hn[0].view, self.hn[1].view, self.cn[0].view, self.cn[1].view,
                     v(self.gates[0]), v(self.gates[1]), v(self.cst[0]), v(self.cst[1]), v(self.hprev[0]), v(self.hprev[1]),
                     v(self.dy), v(self.dm), DROP_P if drop else 0.0, self.seed, salt]

    def desc(self):
        from mmego_amd import hip
        c, P = self.args, hip.pair2
        return hip.Lstm64Fwd(P(c[2], c[3]), c[4], P(c[5], c[6]), P(c[7], c[8]), P(c[9], c[10]), P(c[11], c[12]), hip.ptr(c[13]), c[14],
                             P(c[15], c[16]), P(c[17], c[18]), P(c[19], c[20]), P(c[21], c[22]), P(c[23], c[24]), c[0], c[1],
                             hip.ptr(c[25]), hip.ptr(c[26]), c[27], hip.ptr(c[28]), c[29])

    def run(self):
        call("lstm64_forward", *self.args)
        return self

    def outputs(self):
        """Everything the call wrote, on the CPU."""
        B, T = self.B, self.T
        r = {"out": self.out.cpu().reshape(B, T, 128), "hn": [h.cpu() for h in self.hn], "cn": [c.cpu() for c in self.cn]}
        if self.stash:
            r["gates"] = [g.cpu().reshape(T, B, 64, 4) for g in self.gates]
            r["cst"] = [c.cpu().reshape(T, B, 64) for c in self.cst]
            r["hprev"] = [h.cpu().reshape(B, T, 64) for h in self.hprev]
        if self.drop:
            r["dy"], r["dm"] = self.dy.cpu().reshape(B, T, 128), self.dm.cpu().reshape(B, T, 128)
        return r

    def guards(self):
        every = [self.xp, self.out] + self.hn + self.cn + [w for w in self.gates + self.cst + self.hprev + [self.dy, self.dm] if w is not None]
        return all(w.guards_intact() for w in every)

    def given(self, key):
        """The fp32 inputs the kernel read for h0 / c0 / b_hh (None where NULL was passed)."""
        if key == "b":
            return self.I["b"]
        return [self.I[key][d] if self.o[key][d] else None for d in range(2)]


l64_opts = R.l64_opts


def check_l64_stepwise(k, I, run, got, note):
    """The stash form, step by step from the kernel's own state."""
    B, T = run.B, run.T
    b, h0, c0 = run.given("b"), run.given("h0"), run.given("c0")
    for d in range(2):
        order = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        for s, t in enumerate(order):
            own = got["out"][:, order[s - 1], d * 64:(d + 1) * 64] if s > 0 else (torch.zeros(B, 64) if h0[d] is None else h0[d])
            assert same_bits(got["hprev"][d][:, t], own), (k, "hprev is not the kernel's own neighbouring out / h0", d, t, note)
            cp = got["cst"][d][order[s - 1]] if s > 0 else (torch.zeros(B, 64) if c0[d] is None else c0[d])
            st = R.step(I["xp"][d][:, t], b[d], got["hprev"][d][:, t], I["W"][d], cp, "lstm64")
            check(k, "gates", got["gates"][d][t].permute(0, 2, 1).reshape(B, 256), *st["gates"], note)
            check(k, "cst", got["cst"][d][t], *st["c"], note)
            check(k, "out", got["out"][:, t, d * 64:(d + 1) * 64], *st["h"], note)
        assert same_bits(got["hn"][d], got["out"][:, order[-1], d * 64:(d + 1) * 64]) and same_bits(got["cn"][d], got["cst"][d][order[-1]]), (k, "hn / cn", note)


def check_l64_chain(k, I, run, got, note):
    ref = R.seq_fwd(I["xp"], I["W"], run.given("b"), run.given("h0"), run.given("c0"))
    check(k, "out", got["out"], *ref["out"], note)
    for d in range(2):
        check(k, "hn", got["hn"][d], *ref["hn"][d], note)
        check(k, "cn", got["cn"][d], *ref["cn"][d], note)
    return ref


@pytest.mark.parametrize("T", R.L64_T)
@pytest.mark.parametrize("B", R.L64_B)
def test_lstm64_forward(dev, B, T):
    """All four <STASH, DROP> forms per shape (B = 16: FULL), options by l64_opts; B = 1 once per row kind."""
    for shift in ((0, 1, 2) if B == 1 else (0,)):
        o = l64_opts(B, T, shift)
        I = R.seq_inputs(B, T, shift, with_b=o["bhh"])
        got = {}
        for stash in (0, 1):
            for drop in (0, 1):
                note = (B, T, shift, stash, drop, R.l64_inst(B, stash, drop))
                run = L64(dev, I, B, T, o, stash, drop).run()
                g = got[(stash, drop)] = run.outputs()
                assert run.guards(), ("guards", note)
                if stash:
                    check_l64_stepwise("lstm64_fwd stash", I, run, g, note)
                else:
                    check_l64_chain("lstm64_fwd chain", I, run, g, note)
                if drop:
                    assert same_bits(g["dy"], g["out"] * g["dm"]), ("drop_y is not out * drop_mask", note)
                    assert bool(((g["dm"] == 0) | (g["dm"] == 1.0 / (1.0 - DROP_P))).all()), note
                    assert same_bits(g["out"], got[(stash, 0)]["out"]), ("out with and without dropout", note)
                    for d in range(2):
                        assert same_bits(g["hn"][d], got[(stash, 0)]["hn"][d]) and same_bits(g["cn"][d], got[(stash, 0)]["cn"][d]), note


class L64B:
    """One mmego_lstm64_backward call."""

    def __init__(self, dev, I, B, T, o, gates, cst):
        from mmego_amd import hip
        self.B, self.T = B, T
        self.dout = Wide(dev, B * T, 128, o["dos"], col=64 if o["dos"] == 256 else 0, fill=NAN, src=I["dout"])
        self.gates = [Wide(dev, T * B, 256, 256, fill=NAN, src=g) for g in gates]
        self.cst = [Wide(dev, T * B, 64, 64, fill=NAN, src=c) for c in cst]
        self.c0 = [d_vec(dev, I["c0"][d]) if o["bc0"][d] else None for d in range(2)]
        self.W = [d_vec(dev, w) for w in I["W"]]
        self.dg = Wide(dev, B * T, 512, o["dgs"])
        self.args = [B, T, self.dout.view, o["dos"], self.gates[0].view, self.gates[1].view, self.cst[0].view, self.cst[1].view, self.c0[0],
                     self.c0[1], self.W[0], self.W[1], self.dg.view, self.dg.view[:, 256:], o["dgs"]]

    def desc(self):
        from mmego_amd import hip
        c, P = self.args, hip.pair2
        return hip.Lstm64Bwd(hip.ptr(c[2]), c[3], P(c[4], c[5]), P(c[6], c[7]), P(c[8], c[9]), P(c[10], c[11]), P(c[12], c[13]), c[14], c[0], c[1])

    def run(self):
        call("lstm64_backward", *self.args)
        return self

    def result(self):
        g = self.dg.cpu().reshape(self.B, self.T, 512)
        return [g[:, :, :256], g[:, :, 256:]]


def check_l64_backward(dev, I, B, T, o, gates, cst, note):
    run = L64B(dev, I, B, T, o, gates, cst).run()
    got = run.result()
    assert run.dg.guards_intact() and run.dout.guards_intact(), ("guards", note)
    c0 = [I["c0"][d] if o["bc0"][d] else None for d in range(2)]
    ref = R.seq_bwd(I["dout"], gates, cst, c0, I["W"], "fast")
    for d in range(2):
        check("lstm64_bwd", "dgates%d" % d, got[d], *ref[d], note)


@pytest.mark.parametrize("T", R.L64_T)
@pytest.mark.parametrize("B", R.L64_B)
def test_lstm64_backward(dev, B, T):
    """Stashes written by the forward kernel; every dgates element of both directions against the bound-carrying chain (exact tanh of the
    stashed c in the reference, the kernel's fast_tanh in the bound)."""
    for shift in ((0, 1, 2) if B == 1 else (0,)):
        o = l64_opts(B, T, shift)
        I = R.seq_inputs(B, T, shift, with_b=o["bhh"])
        fo = dict(o, c0=o["bc0"])           # the forward that wrote the stashes started from the c0 the backward is given
        f = L64(dev, I, B, T, fo, 1, 0).run().outputs()
        check_l64_backward(dev, I, B, T, o, f["gates"], f["cst"], (B, T, shift, "kernel stashes"))


@pytest.mark.parametrize("B,T", ((17, 5), (16, 2)))
def test_lstm64_backward_from_reference_stashes(dev, B, T):
    """Stashes written by the float64 reference, rounded to fp32: a forward error cannot hide a backward one."""
    I, o = R.seq_inputs(B, T), OPTS[0]
    c0 = [I["c0"][d] if o["bc0"][d] else None for d in range(2)]
    ref = R.seq_fwd(I["xp"], I["W"], I["b"], I["h0"], c0)
    check_l64_backward(dev, I, B, T, o, [g.float() for g in ref["gates"]], [c.float() for c in ref["cst"]], (B, T, "reference stashes"))


@pytest.mark.parametrize("n", (1, 3, 4))
def test_lstm64_multi(dev, n):
    """n stacks in one launch (grid z = stack) give the bits of n single launches, forward (stash + dropout, and the plain form) and
    backward; mixed options across stacks are refused."""
    from mmego_amd import hip
    B, T = 17, 2
    Is = [R.seq_inputs(B, T, 10 + i, with_b=OPTS[i % 4]["bhh"]) for i in range(n)]
    for stash, drop in ((1, 1), (0, 0)):
        single = [L64(dev, Is[i], B, T, OPTS[i % 4], stash, drop, salt=i).run() for i in range(n)]
        multi = [L64(dev, Is[i], B, T, OPTS[i % 4], stash, drop, salt=i) for i in range(n)]
        call("lstm64_forward_multi", n, (hip.Lstm64Fwd * n)(*[m.desc() for m in multi]))
        for i in range(n):
            a, b = single[i].outputs(), multi[i].outputs()
            assert multi[i].guards(), i
            for key in a:
                for x, y in zip(a[key] if isinstance(a[key], list) else [a[key]], b[key] if isinstance(b[key], list) else [b[key]]):
                    assert same_bits(x, y), (n, i, key, stash, drop)
    f = [L64(dev, Is[i], B, T, dict(OPTS[i % 4], c0=OPTS[i % 4]["bc0"]), 1, 0).run().outputs() for i in range(n)]
    sb = [L64B(dev, Is[i], B, T, OPTS[i % 4], f[i]["gates"], f[i]["cst"]).run() for i in range(n)]
    # (one dgs per launch is no requirement of the ABI: every stack brings its own strides)
    mb = [L64B(dev, Is[i], B, T, OPTS[i % 4], f[i]["gates"], f[i]["cst"]) for i in range(n)]
    call("lstm64_backward_multi", n, (hip.Lstm64Bwd * n)(*[m.desc() for m in mb]))
    for i in range(n):
        assert mb[i].dg.guards_intact() and same_bits(sb[i].dg.view, mb[i].dg.view), (n, i)
    if n >= 3:
        for stash2, drop2 in ((0, 1), (1, 0)):        # stack 1 without the stashes / without the dropout of the others
            mixed = [L64(dev, Is[i], B, T, OPTS[0], 1 if i != 1 else stash2, 1 if i != 1 else drop2, salt=i) for i in range(n)]
            refused("lstm64_forward_multi", n, (hip.Lstm64Fwd * n)(*[m.desc() for m in mixed]))
            assert all(m.out.guards_intact() and bool((m.out.view == SENT).all()) for m in mixed)
    refused("lstm64_forward_multi", 0, (hip.Lstm64Fwd * 1)(multi[0].desc()))
    refused("lstm64_forward_multi", 5, (hip.Lstm64Fwd * 5)(*[multi[0].desc()] * 5))


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_lstm_step
# ---------------------------------------------------------------------------------------------------------------------------------
KIND = {"lstm_first_step_kernel": "first", "lstm_step_dma_kernel": "dma", "lstm_step_small_kernel": "small"}


class Step:
    """One mmego_lstm_step call in the production layout: hps = hos = 2H, xs = 8H, the other direction's columns NaN (operands) or the
    sentinel (h out); c in place; boff: b_hh one float past an aligned address."""

    def __init__(self, dev, I, ndir, Bn, H, first, boff, stash=True):
        self.ndir, self.Bn, self.H = ndir, Bn, H
        z = [None, None]
        self.hp = [Wide(dev, Bn, H, 2 * H, col=d * H, fill=NAN, src=I["h"][d]) if not first else None for d in range(ndir)] + z
        self.xp = [Wide(dev, Bn, 4 * H, 8 * H, col=d * 4 * H, fill=NAN, src=I["xp"][d]) for d in range(ndir)] + z
        self.W = [d_vec(dev, I["W"][d]) for d in range(ndir)] + z
        self.b = [Wide(dev, 1, 4 * H, 4 * H, fill=NAN, src=I["b"][d], lead=boff, guard=1) for d in range(ndir)] + z
        self.ho = [Wide(dev, Bn, H, 2 * H, col=d * H) for d in range(ndir)] + z
        self.c = [dense(dev, torch.zeros(Bn, H) if first else I["c"][d]) for d in range(ndir)] + z
        self.gst = [Wide(dev, Bn, 4 * H, 4 * H) if stash else None for d in range(ndir)] + z
        self.cst = [Wide(dev, Bn, H, H) if stash else None for d in range(ndir)] + z
        v = lambda w: None if w is None else w.view
        self.args = [ndir, Bn, H, first, v(self.hp[0]), v(self.hp[1]), 2 * H, self.W[0], self.W[1], v(self.b[0]), v(self.b[1]), v(self.xp[0]),
                     v(self.xp[1]), 8 * H, v(self.ho[0]), v(self.ho[1]), 2 * H, v(self.c[0]), v(self.c[1]), v(self.gst[0]), v(self.gst[1]),
                     v(self.cst[0]), v(self.cst[1])]

    def run(self):
        call("lstm_step", *self.args)
        return self

    def guards(self):
        return all(w.guards_intact() for w in self.hp + self.xp + self.ho + self.c + self.gst + self.cst + self.b if w is not None)


def check_step(dev, case, I=None):
    ndir, Bn, H, first, boff, kernel = case
    I = I or R.step_inputs(ndir, Bn, H)
    run = Step(dev, I, ndir, Bn, H, first, boff).run()
    assert run.guards(), ("guards", case)
    k = kernel.replace("lstm_step_", "").replace("lstm_", "").replace("_kernel", "") + (" first" if first and "first" not in kernel else "")
    for d in range(ndir):
        ref = R.step(I["xp"][d], I["b"][d], I["h"][d], I["W"][d], I["c"][d], "first" if first else KIND[kernel.split("<")[0]])
        check(k, "gates", run.gst[d].cpu(), *ref["gates"], case)
        check(k, "c", run.c[d].cpu(), *ref["c"], case)
        check(k, "h", run.ho[d].cpu(), *ref["h"], case)
        assert same_bits(run.cst[d].view, run.c[d].view), ("cst is not c", case)
    return run


@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: "-".join(str(v) for v in c[:5]))
def test_lstm_step(dev, case):
    """h, c, all four stashed gates and cst of every kernel and instantiation (tests/test_lstm_ref_cpu.py pins which one a case reaches).
    lstm_step_dma_kernel at H = 32 .. 128 holds nk = 1 .. 4 chunks in its three-stage ring.  Barrier count, read from the kernel for
    nk = 0 (first), 1, 2, 3, 4: loader waves run barrier (1), one barrier per kt in [0, nk - 1) and barrier (E): nk + 1 (2 when first);
    compute waves run barrier (1), one barrier per kt with kt + 1 < nk and the __syncthreads (E): nk + 1 (2 when first) -- equal for every
    nk.  The output tile OUT = stage nk % 3 is never a stage still in use: chunk nk - 1 sits in stage (nk - 1) % 3, and every wave's reads
    of the chunk that used stage nk % 3 last (chunk nk - 3) are behind barrier B_{nk-3}.  Loader rows past Bn are clamped to a valid row."""
    ndir, Bn, H, first, boff, kernel = case
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if "dma" in kernel:
        assert R.step_kernel(bool(first), not boff, ndir, Bn, H, ncu) == kernel, ("the device's CU count sends this case elsewhere", ncu)
    run = check_step(dev, case)
    if first and boff:
        # the first step through a general kernel: the bits of the first-step kernel except for the sign of a zero c
        I = R.step_inputs(ndir, Bn, H)
        f = Step(dev, I, ndir, Bn, H, 1, 0).run()
        for d in range(ndir):
            assert same_bits(run.gst[d].view, f.gst[d].view) and same_bits(run.ho[d].view, f.ho[d].view), case
            assert torch.equal(run.c[d].cpu(), f.c[d].cpu()), case
            nz = run.c[d].cpu() != 0
            assert same_bits(run.c[d].cpu()[nz], f.c[d].cpu()[nz]), case


def test_lstm_step_dma32(dev):
    """lstm_step_dma_kernel<32> at H = 512 with the smallest ragged Bn (64 n + 8) at which 2 * grid32 exceeds the device's CU count."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    Bn = R.smallest_dma32_bn(2, 512, ncu)
    assert R.step_kernel(False, True, 2, Bn, 512, ncu) == "lstm_step_dma_kernel<32>" and Bn % 64 == 8
    assert R.step_kernel(False, True, 2, Bn - 64, 512, ncu) == "lstm_step_dma_kernel<16>"
    check_step(dev, (2, Bn, 512, 0, 0, "lstm_step_dma_kernel<32>"))


def test_lstm_step_without_stash_and_one_direction(dev):
    """No stash (gst / cst NULL) gives the same h and c; ndir = 1 leaves direction 1's pointers unread (NULL)."""
    for case in ((1, 136, 64, 0, 0, "lstm_step_dma_kernel<16>"), (2, 37, 96, 0, 0, "lstm_step_small_kernel<32, false>")):
        ndir, Bn, H = case[:3]
        I = R.step_inputs(ndir, Bn, H)
        a, b = Step(dev, I, ndir, Bn, H, 0, 0).run(), Step(dev, I, ndir, Bn, H, 0, 0, stash=False).run()
        assert b.guards()
        for d in range(ndir):
            assert same_bits(a.ho[d].view, b.ho[d].view) and same_bits(a.c[d].view, b.c[d].view), case


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_lstm_cell_backward, mmego_lstm_bwd_step
# ---------------------------------------------------------------------------------------------------------------------------------
TB = 2          # time steps of the production buffers the slices are cut from


@pytest.mark.parametrize("case", R.CELL_BWD_CASES, ids=str)
def test_lstm_cell_backward(dev, case):
    """dout and dgates as time slices of [Bn][T * 2H] / [Bn][T * 8H]; gst with its fixed row stride 4H; dc in place; dhrec / cprev given
    or NULL."""
    ndir, Bn, H = case
    I = R.bwd_inputs(ndir, Bn, H)
    z = [None, None]
    for rec in (0, 1):
        for cpv in (0, 1):
            t = (rec + cpv) % TB
            dout = [Wide(dev, Bn, H, TB * 2 * H, col=t * 2 * H + d * H, fill=NAN, src=I["dout"][d]) for d in range(ndir)] + z
            dg = [Wide(dev, Bn, 4 * H, TB * 8 * H, col=t * 8 * H + d * 4 * H) for d in range(ndir)] + z
            dhr = [d_vec(dev, I["dhrec"][d]) if rec else None for d in range(ndir)] + z
            gst = [d_vec(dev, I["gst"][d]) for d in range(ndir)] + z
            cst = [d_vec(dev, I["cst"][d]) for d in range(ndir)] + z
            cp = [d_vec(dev, I["cprev"][d]) if cpv else None for d in range(ndir)] + z
            dc = [dense(dev, I["dc"][d]) for d in range(ndir)] + z
            v = lambda w: None if w is None else w.view
            call("lstm_cell_backward", ndir, Bn, H, v(dout[0]), v(dout[1]), TB * 2 * H, dhr[0], dhr[1], gst[0], gst[1], cst[0], cst[1], cp[0], cp[1],
                 v(dc[0]), v(dc[1]), v(dg[0]), v(dg[1]), TB * 8 * H)
            for d in range(ndir):
                g, dh = I["gst"][d], I["dout"][d].double() + (I["dhrec"][d].double() if rec else 0.0)
                ref = R.cell_bwd(g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:], I["cst"][d], I["cprev"][d] if cpv else None, I["dc"][d], dh,
                                 0.0, R.U32 * dh.abs() if rec else 0.0, "libm")
                note = (case, rec, cpv, d)
                check("cell_bwd", "dgates", dg[d].cpu(), *R.dgates_of(ref), note)
                check("cell_bwd", "dc", dc[d].cpu(), *ref["dcprev"], note)
                assert dg[d].guards_intact() and dc[d].guards_intact() and dout[d].guards_intact(), note


def run_bwd_step(dev, I, Bn, H, cpv):
    """dg (step 1) and dgo (step 0) as two time slices of one [Bn][T][8H] buffer, as imu_train.py passes them -> (dgo [2], dc [2])."""
    big = Wide(dev, Bn, TB * 8 * H, TB * 8 * H)
    dgn = [big.view[:, 8 * H + d * 4 * H:8 * H + (d + 1) * 4 * H] for d in range(2)]
    dgo = [big.view[:, d * 4 * H:(d + 1) * 4 * H] for d in range(2)]
    for d in range(2):
        dgn[d].copy_(I["dgn"][d])
    wT = [d_vec(dev, I["W"][d].t().contiguous()) for d in range(2)]
    dout = [Wide(dev, Bn, H, TB * 2 * H, col=d * H, fill=NAN, src=I["dout"][d]) for d in range(2)]
    gst, cst = [d_vec(dev, I["gst"][d]) for d in range(2)], [d_vec(dev, I["cst"][d]) for d in range(2)]
    cp = [d_vec(dev, I["cprev"][d]) if cpv else None for d in range(2)]
    dc = [dense(dev, I["dc"][d]) for d in range(2)]
    call("lstm_bwd_step", Bn, H, dgn[0], dgn[1], TB * 8 * H, wT[0], wT[1], dout[0].view, dout[1].view, TB * 2 * H, gst[0], gst[1], cst[0], cst[1],
         cp[0], cp[1], dc[0].view, dc[1].view, dgo[0], dgo[1])
    assert big.guards_intact() and all(w.guards_intact() for w in dc + dout), ("guards", Bn, H)
    for d in range(2):
        assert same_bits(dgn[d], I["dgn"][d]), "the step's input slice was written"
    return [g.cpu() for g in dgo], [c.cpu() for c in dc]


@pytest.mark.parametrize("case", R.BWD_STEP_CASES, ids=lambda c: "-".join(str(v) for v in c[:3]))
def test_lstm_bwd_step(dev, case, monkeypatch):
    """Every dgo and dc element of both directions against float64; the LDS-DMA form at K = 4H = 2 .. 8 chunks (and 32), the K-quartered form
    at Bn = 32, 96 and, switched by MMEGO_LSTM_BWD_DMA=0, at 64; cprev given and NULL."""
    Bn, H, env, kernel = case
    if env is not None:
        monkeypatch.setenv("MMEGO_LSTM_BWD_DMA", env)
    I = R.bwd_inputs(2, Bn, H)
    k = "bwd_step dma" if "dma" in kernel else "bwd_step kq"
    for cpv in (1, 0):
        dgo, dc = run_bwd_step(dev, I, Bn, H, cpv)
        for d in range(2):
            ref = R.bwd_step(I["dgn"][d], I["W"][d], I["dout"][d], I["gst"][d], I["cst"][d], I["cprev"][d] if cpv else None, I["dc"][d],
                             0 if "dma" in kernel else 3)
            check(k, "dgo", dgo[d], *R.dgates_of(ref), (case, cpv, d))
            check(k, "dc", dc[d], *ref["dcprev"], (case, cpv, d))


@pytest.mark.parametrize("Bn,H", ((64, 64), (128, 96)))
def test_lstm_bwd_step_forms_agree(dev, Bn, H, monkeypatch):
    """The LDS-DMA form and the K-quartered form differ in the product's summation order alone: their difference is inside the bound of
    one of them (the product bound of the longer chain plus the cell backward's roundings), not twice it."""
    I = R.bwd_inputs(2, Bn, H)
    a = run_bwd_step(dev, I, Bn, H, 1)
    monkeypatch.setenv("MMEGO_LSTM_BWD_DMA", "0")
    b = run_bwd_step(dev, I, Bn, H, 1)
    for d in range(2):
        ref = R.bwd_step(I["dgn"][d], I["W"][d], I["dout"][d], I["gst"][d], I["cst"][d], I["cprev"][d], I["dc"][d], 3)
        check("bwd_step dma - kq", "dgo", a[0][d], b[0][d].double(), R.dgates_of(ref)[1], (Bn, H, d))
        check("bwd_step dma - kq", "dc", a[1][d], b[1][d].double(), ref["dcprev"][1], (Bn, H, d))


# ---------------------------------------------------------------------------------------------------------------------------------
# mmego_imu_loss, mmego_imu_head, mmego_imu_head_backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", R.IMU_F)
def test_imu_loss(dev, F):
    """Loss and both gradients; frames with R == R_gt (the clamped cosine: exactly zero gradient), with t == head (norm 0: exactly zero
    gradient) and ordinary rotations; F past the single block's 1024 threads; dR and dt NULL."""
    inp = R.imu_loss_inputs(F)
    ops_ = [d_vec(dev, x) for x in inp]
    (loss, e_loss), (dR, e_dR), (dt, e_dt) = R.imu_loss(*inp, 0.25)
    o_l, o_R, o_t = Out(dev, 1, 1, strided=False), Out(dev, F, 9, strided=False), Out(dev, F, 3, strided=False)
    call("imu_loss", *ops_, F, 0.25, o_l.view, o_R.view, o_t.view)
    check("imu_loss", "loss", o_l.cpu().view(()), loss, e_loss, F)
    check("imu_loss", "dR", o_R.cpu(), dR, e_dR, F)
    check("imu_loss", "dt", o_t.cpu(), dt, e_dt, F)
    got_R, got_t = o_R.cpu(), o_t.cpu()
    for f in range(min(F, 8)):
        assert f % 4 != 1 or bool((got_R[f] == 0).all())
        assert f % 4 != 2 or bool((got_t[f] == 0).all())
    assert o_l.guards_intact() and o_R.guards_intact() and o_t.guards_intact()
    o_l2 = Out(dev, 1, 1, strided=False)
    call("imu_loss", *ops_, F, 0.25, o_l2.view, None, None)
    assert same_bits(o_l2.view, o_l.view) and o_l2.guards_intact()


@pytest.mark.parametrize("F", R.IMU_F)
def test_imu_head_and_backward(dev, F):
    """The 6-D head and its backward against float64 (autograd of the restated forward); ordinary y, a zero first vector and parallel
    vectors (the <= eps branches)."""
    y, dR, dt = R.imu_head_inputs(F)
    yd, dRd, dtd = d_vec(dev, y), d_vec(dev, dR), d_vec(dev, dt)
    (Rr, eR), (tr, et) = R.imu_head(y)
    o_R, o_t, o_y = Out(dev, F, 9, strided=False), Out(dev, F, 3, strided=False), Out(dev, F, 9, strided=False)
    call("imu_head", yd, F, o_R.view, o_t.view)
    check("imu_head", "R", o_R.cpu(), Rr, eR, F)
    check("imu_head", "t", o_t.cpu(), tr, et, F)
    ref, e = R.imu_head_bwd(y, dR, dt)
    call("imu_head_backward", yd, dRd, dtd, F, o_y.view)
    check("imu_head_bwd", "dy", o_y.cpu(), ref, e, F)
    assert o_R.guards_intact() and o_t.guards_intact() and o_y.guards_intact()


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """Every MMEGO_REQUIRE of these entry points a caller could plausibly trip returns MMEGO_EBADARG without a launch."""
    from mmego_amd import hip
    # mmego_lstm_step
    ndir, Bn, H = 2, 37, 96
    I = R.step_inputs(ndir, Bn, H)

    def step_args(**kw):
        a = list(Step(dev, I, ndir, Bn, H, kw.pop("first", 0), 0).args)
        names = ["ndir", "Bn", "H", "first", "hp0", "hp1", "hps", "W0", "W1", "b0", "b1", "xp0", "xp1", "xs", "ho0", "ho1", "hos", "c0", "c1", "gst0",
                 "gst1", "cst0", "cst1"]
        for k_, v_ in kw.items():
            a[names.index(k_)] = v_
        return a
    base = step_args()
    call("lstm_step", *base)                                   # (the unmodified list is accepted)
    off1 = lambda t: torch.cat((t.reshape(-1), t.new_zeros(8)))[1:]          # the same size, 4 bytes past an aligned address
    for bad in (dict(H=48), dict(H=0), dict(ndir=3), dict(ndir=0), dict(Bn=0), dict(cst0=None), dict(gst1=None), dict(xs=8 * H + 2), dict(hos=2 * H + 2),
                dict(hps=2 * H + 1), dict(hp0=None), dict(hp1=None), dict(W1=None), dict(xp1=None), dict(c1=None), dict(ho1=None),
                dict(W0=off1(base[7])), dict(W1=off1(base[8])), dict(xp0=off1(base[11])), dict(c0=off1(base[17])), dict(ho1=off1(base[15])),
                dict(hp1=off1(base[5]))):
        refused("lstm_step", *step_args(**bad))
    # mmego_lstm_cell_backward
    J = R.bwd_inputs(2, 37, 32)
    t = {k_: [d_vec(dev, x) for x in J[k_]] for k_ in ("dout", "gst", "cst", "dc")}
    dg = [d_vec(dev, torch.zeros(37, 128)) for _ in range(2)]

    def cb(nd=2, Bn=37, H=32, dout1=t["dout"][1], gst0=t["gst"][0], cst1=t["cst"][1], dc1=t["dc"][1], dg1=dg[1]):
        return [nd, Bn, H, t["dout"][0], dout1, 32, None, None, gst0, t["gst"][1], t["cst"][0], cst1, None, None, t["dc"][0], dc1, dg[0], dg1, 128]
    for bad in (dict(nd=0), dict(nd=3), dict(Bn=0), dict(H=0), dict(dout1=None), dict(gst0=None), dict(cst1=None), dict(dc1=None), dict(dg1=None)):
        refused("lstm_cell_backward", *cb(**bad))
    # mmego_lstm_bwd_step
    K = R.bwd_inputs(2, 64, 32)
    u = {k_: [d_vec(dev, x) for x in K[k_]] for k_ in ("dout", "gst", "cst", "dc", "dgn", "cprev")}
    wT = [d_vec(dev, w.t().contiguous()) for w in K["W"]]
    dgo = [d_vec(dev, torch.zeros(64, 128)) for _ in range(2)]

    def bs(Bn=64, H=32, dg0=u["dgn"][0], dg1=u["dgn"][1], dgs=128, w0=wT[0], cp0=None, cp1=None, dc1=u["dc"][1], dgo1=dgo[1]):
        return [Bn, H, dg0, dg1, dgs, w0, wT[1], u["dout"][0], u["dout"][1], 32, u["gst"][0], u["gst"][1], u["cst"][0], u["cst"][1], cp0, cp1,
                u["dc"][0], dc1, dgo[0], dgo1]
    for bad in (dict(Bn=40), dict(Bn=0), dict(H=48), dict(dgs=130), dict(cp0=u["cprev"][0]), dict(cp1=u["cprev"][1]), dict(dg1=None), dict(dc1=None),
                dict(dgo1=None), dict(dg0=off1(u["dgn"][0])), dict(dg1=off1(u["dgn"][1])), dict(w0=off1(wT[0]))):
        refused("lstm_bwd_step", *bs(**bad))
    # stage-1 loss and head
    li = [d_vec(dev, x) for x in R.imu_loss_inputs(6)]
    o1, o9, o3 = d_vec(dev, torch.zeros(1)), d_vec(dev, torch.zeros(6, 9)), d_vec(dev, torch.zeros(6, 3))
    for bad in ([None] + li[1:] + [6, 1.0, o1, o9, o3], li + [0, 1.0, o1, o9, o3], li + [6, 1.0, None, o9, o3], li[:3] + [None, 6, 1.0, o1, o9, o3]):
        refused("imu_loss", *bad)
    for bad in ((None, 6, o9, o3), (o9, 0, o9, o3), (o9, 6, None, o3), (o9, 6, o9, None)):
        refused("imu_head", *bad)
    for bad in ((None, o9, o3, 6, o9), (o9, None, o3, 6, o9), (o9, o9, None, 6, o9), (o9, o9, o3, 0, o9), (o9, o9, o3, 6, None)):
        refused("imu_head_backward", *bad)
    # mmego_lstm64_forward / _backward and the _multi forms
    B, T = 13, 2
    S = R.seq_inputs(B, T)
    names = ["B", "T", "xp0", "xp1", "xs", "W0", "W1", "b0", "b1", "h00", "h01", "c00", "c01", "out", "os", "hn0", "hn1", "cn0", "cn1", "gates0", "gates1",
             "cst0", "cst1", "hprev0", "hprev1", "dy", "dm", "p", "seed", "salt"]

    def fwd(**kw):
        r = L64(dev, S, B, T, OPTS[0], 1, 1)
        for k_, v_ in kw.items():
            r.args[names.index(k_)] = v_(r) if callable(v_) else v_
        return r
    for bad in (dict(B=0), dict(T=0), dict(xp1=None), dict(out=None), dict(W0=lambda r: off1(r.W[0])), dict(cst0=None), dict(gates1=None), dict(hprev0=None),
                dict(hprev1=None), dict(gates0=None, cst0=None), dict(dy=None), dict(dm=None), dict(seed=None), dict(p=0.0), dict(p=1.0),
                # the gate stash is stored 16 bytes at a time: a base 4 bytes past an aligned address is refused
                dict(gates0=lambda r: off1(r.gates[0].view)), dict(gates1=lambda r: off1(r.gates[1].view))):
        r = fwd(**bad)
        refused("lstm64_forward", *r.args)
        refused("lstm64_forward_multi", 1, (hip.Lstm64Fwd * 1)(r.desc()))
        assert bool((r.out.buf == SENT).all())
    f = L64(dev, S, B, T, OPTS[0], 1, 0).run().outputs()
    bn = ["B", "T", "dout", "dos", "gates0", "gates1", "cst0", "cst1", "c00", "c01", "W0", "W1", "dg0", "dg1", "dgs"]
    for bad in (dict(B=0), dict(T=0), dict(dout=None), dict(gates1=None), dict(cst0=None), dict(dg1=None), dict(W1=lambda r: off1(r.W[1])),
                dict(gates0=lambda r: off1(r.gates[0].view)), dict(gates1=lambda r: off1(r.gates[1].view))):
        r = L64B(dev, S, B, T, OPTS[0], f["gates"], f["cst"])
        for k_, v_ in bad.items():
            r.args[bn.index(k_)] = v_(r) if callable(v_) else v_
        refused("lstm64_backward", *r.args)
        refused("lstm64_backward_multi", 1, (hip.Lstm64Bwd * 1)(r.desc()))
        assert bool((r.dg.buf == SENT).all())
    refused("lstm64_backward_multi", 0, (hip.Lstm64Bwd * 1)(r.desc()))
    refused("lstm64_backward_multi", 5, (hip.Lstm64Bwd * 5)(*[r.desc()] * 5))
