"""CPU: the float64 reference, the bound, the dispatch restatement and the case table of tests/gemm_ref.py, which
tests/test_gemm_kernels_gpu.py runs against the fp32 GEMM kernels -- checked here without a GPU, so that a mistake in the yardstick
does not hide behind the kernels it measures."""
import os
import re

import pytest
import torch

import gemm_ref as R
from mmego_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ENTRIES = R.CASES + [c for _, _, cs in R.GROUPS for c in cs]


def test_thresholds_are_the_sources():
    src = open(os.path.join(ROOT, "mmego_amd", "csrc", "gemm.hip")).read()
    const = lambda name: int(re.search(r"(?:constexpr \w+|#define) %s(?: =)? (\d+)" % name, src).group(1))
    assert ops._TILE_MIN_OTHER == const("GEMM_TILE_MIN_OTHER")
    assert ops._KQ_MAX == const("GEMM_KQ_MAX")
    assert R.GROUP_MAX == const("GEMM_GROUP_MAX")


def dense(c, bufs):
    """A [nb][M][K], B [nb][K][N] gathered element by element through the header's index maps (no strided views)."""
    L = R.Layout(c)
    b, m, k, n = (torch.arange(x) for x in (c.nbatch, c.M, c.K, c.N))
    ia = L.offA + b[:, None, None] * L.sAb + m[None, :, None] * L.sam + k[None, None, :] * L.sak
    ib = L.offB + b[:, None, None] * L.sBb + k[None, :, None] * L.sbk + n[None, None, :] * L.sbn
    return bufs["A"][ia].double(), bufs["B"][ib].double()


@pytest.mark.parametrize("orient", ["NN", "NT", "TN", "TT"])
@pytest.mark.parametrize("nbatch", [1, 3])
def test_ref_is_matmul_on_plain_forms(orient, nbatch):
    c = R.Case("plain_" + orient, "kq", 9, 7, 70, orient, nbatch=nbatch, gap=nbatch > 1)
    for kind in ("int", "normal"):
        bufs = R.make_bufs(c, kind)
        A, B = dense(c, bufs)
        assert not torch.isnan(A).any() and not torch.isnan(B).any()
        want = torch.matmul(A, B)
        got = R.ref(c, bufs)
        assert torch.equal(got["C"], want) if kind == "int" else torch.allclose(got["C"], want, rtol=1e-13, atol=1e-13)
        assert torch.equal(got["prod"], got["C"]) and got["asum"] is None


def loop_ref(c, bufs):
    """The contract as loops over the flat storage, python floats (float64)."""
    L = R.Layout(c)
    f = {k: (v.tolist() if v is not None else None) for k, v in bufs.items()}
    C = [[[None] * c.N for _ in range(c.M)] for _ in range(c.nbatch)]
    S = [[None] * c.M for _ in range(c.nbatch)]
    for b in range(c.nbatch):
        for m in range(c.M):
            rs = 0.0
            for k in range(c.K):
                rs += f["A"][L.offA + b * L.sAb + m * L.sam + k * L.sak]
            S[b][m] = rs + (f["asum"][R.GUARD + b * c.M + m] if c.asum and c.accumulate == 1 else 0.0)
            for n in range(c.N):
                s = 0.0
                for k in range(c.K):
                    s += f["A"][L.offA + b * L.sAb + m * L.sam + k * L.sak] * f["B"][L.offB + b * L.sBb + k * L.sbk + n * L.sbn]
                ic = L.offC + b * L.sCb + m * L.scm + n * L.scn
                if c.bias:
                    s += f["bias"][R.GUARD + b * L.sBiasb + n]
                if c.relu == 1:
                    s = max(s, 0.0)
                if c.accumulate == 1:
                    s += f["C"][ic]
                if c.cmul:
                    s = (s if f["cmul"][ic] > 0 else 0.0) if c.relu == 2 else s * f["cmul"][ic]
                C[b][m][n] = s
    return torch.tensor(C, dtype=torch.float64), torch.tensor(S, dtype=torch.float64)


@pytest.mark.parametrize("relu", [1, 2, 0])
def test_ref_is_the_triple_loop_with_every_option(relu):
    c = R.Case("loops%d" % relu, "g64_bk16", 3, 4, 5, "TT", nbatch=2, gap=True, bias_b=True, relu=relu, accumulate=1, cmul=True, asum=True,
               scn=2, misalign=True)
    for kind in ("int", "normal"):
        bufs = R.make_bufs(c, kind)
        wc, ws = loop_ref(c, bufs)
        got = R.ref(c, bufs)
        if kind == "int":
            assert torch.equal(got["C"], wc) and torch.equal(got["asum"], ws)
        else:
            assert torch.allclose(got["C"], wc, rtol=1e-13, atol=1e-13) and torch.allclose(got["asum"], ws, rtol=1e-13, atol=1e-13)
    # relu comes before accumulate: a case where the other order gives another number
    c = R.Case("order", "g64_bk16", 1, 1, 1, accumulate=1, relu=1, bias=True)
    bufs = R.make_bufs(c, "int")
    v = R.views(c, bufs)
    v["A"].fill_(2.0), v["B"].fill_(-3.0), v["bias"].fill_(1.0), v["C"].fill_(4.0)
    assert R.ref(c, bufs)["C"].item() == 4.0              # 4 + relu(-6 + 1), not relu(4 - 6 + 1) = 0


def test_deferred_ref_leaves_c_and_reports_the_product():
    c = R.Case("deferred", "kq", 5, 6, 300, "TN", nsplit=3, accumulate=2, asum=True)
    bufs = R.make_bufs(c, "int")
    got = R.ref(c, bufs)
    A, B = dense(c, bufs)
    assert got["C"] is None and torch.equal(got["prod"], torch.matmul(A, B)) and torch.equal(got["asum"], A.sum(2))
    assert not R.written_mask(c, bufs)["C"].any() and not R.written_mask(c, bufs)["asum"].any()
    assert int(R.written_mask(c, bufs)["ws"].sum()) == 3 * 5 * 6 + 3 * 5


def test_buffers_guard_and_fill():
    c = R.Case("guards", "kq", 5, 6, 70, "NT", nbatch=2, gap=True, scn=2, bias_b=True, asum=True, nsplit=2)
    bufs = R.make_bufs(c, "int")
    L = R.Layout(c)
    for name in ("C", "asum", "ws"):                      # outputs the call overwrites: all sentinel
        assert (bufs[name].view(torch.int32) == R.SENTINEL).all()
    assert torch.isnan(bufs["C"]).all()
    assert int((~torch.isnan(bufs["A"])).sum()) == 2 * 5 * 70 and int((~torch.isnan(bufs["B"])).sum()) == 2 * 6 * 70
    assert int((~torch.isnan(bufs["bias"])).sum()) == 2 * 6
    assert int(R.written_mask(c, bufs)["C"].sum()) == 2 * 5 * 6 and L.scm > 6 * 2 and L.sCb > 5 * L.scm
    assert bufs["ws"].numel() > L.ws_need == 2 * 2 * 5 * 6 + 2 * 2 * 5


def test_integer_sets_are_exact_in_fp32():
    """Every partial sum of every order is an integer below 2^24 in magnitude, and so is the result after the multiplier."""
    for c in ALL_ENTRIES:
        assert 49 * c.K + 14 < 2 ** 24 and 2 * (49 * c.K + 14) < 2 ** 24, c.name
    for c in ALL_ENTRIES[:40]:
        if c.M * c.N * c.nbatch > 100000:
            continue
        bufs = R.make_bufs(c, "int")
        for name, v in R.views(c, bufs).items():
            if name == "C" and not c.accumulate or name == "asum" and c.accumulate != 1:
                continue
            lo, hi = (-1, 2) if name == "cmul" else (-7, 7)
            assert torch.equal(v, v.round()) and lo <= v.min() and v.max() <= hi, (c.name, name)
        got = R.ref(c, bufs)
        for k in ("C", "prod", "asum"):
            if got[k] is not None:
                assert torch.equal(got[k], got[k].float().double()) and got[k].abs().max() < 2 ** 24


@pytest.mark.parametrize("c", ALL_ENTRIES, ids=lambda c: c.name)
def test_fp32_evaluation_lies_inside_the_bound(c):
    bufs = R.make_bufs(c, "normal")
    want, bnd, got = R.ref(c, bufs), R.bound(c, bufs), R.fp32_eval(c, bufs)
    for k in ("C", "prod", "asum"):
        assert (want[k] is None) == (bnd[k] is None) == (got[k] is None)
        if want[k] is not None:
            err = (got[k].double() - want[k]).abs()
            assert bool((err <= R.SECOND_ORDER * bnd[k]).all()), (c.name, k, float((err / bnd[k]).max()))


def test_bound_rejects_a_bf16_operand():
    """What the normal set is for: with A rounded to bf16 most outputs leave the bound, at the K of every path's shortest case."""
    for K in (16, 64, 128, R.PERSIST_MIN_K):
        c = R.Case("bf16_%d" % K, "kq", 64, 64, K, "NT")
        bufs = R.make_bufs(c, "normal")
        want, bnd = R.ref(c, bufs)["C"], R.bound(c, bufs)["C"]
        R.views(c, bufs)["A"].copy_(R.views(c, bufs)["A"].bfloat16().float())
        err = (R.ref(c, bufs)["C"] - want).abs()
        assert float((err > R.SECOND_ORDER * bnd).double().mean()) > 0.9, K
        assert R.bf16_typical_error(K) > 10 * float(bnd.mean())


def test_table_labels_are_the_dispatch():
    names = [c.name for c in ALL_ENTRIES + R.REFUSALS + [c for _, cs in R.GROUP_REFUSALS for c in cs]]
    assert len(names) == len(set(names))
    for c in ALL_ENTRIES + R.REFUSALS:
        assert R.path_of(c) == c.label, (c.name, c.label, R.path_of(c))
    for name, label, cs in R.GROUPS:
        assert R.group_path_of(cs) == label, name
    for name, cs in R.GROUP_REFUSALS:
        assert R.group_path_of(cs) == "refused", name
        assert sum(R.path_of(c) == "refused" for c in cs) == 1


def test_every_path_and_option_is_covered():
    by = {}
    for c in R.CASES:
        by.setdefault(R.kernel_of(c.label), []).append(c)
    assert set(by) == set(R.LABELS)
    for label, cs in by.items():
        assert len(cs) >= 2, label
        kmin = min(c.K for c in cs)
        if label.startswith("persist"):                   # K > 128 is part of what reaches the walk: its shortest K instead
            assert kmin == R.PERSIST_MIN_K, label
        else:
            assert kmin <= 128, label
    assert {c.label for c in R.CASES if "+reduce" in c.label} >= {"g64_bk16+reduce", "g64_bk64+reduce", "kq+reduce", "tile64+reduce"}
    for opt, paths in R.OPTION_PATHS.items():
        for p in paths:
            assert any(opt in c.options for c in by[p]), (opt, p)
    # the options the other paths refuse or hand on: no case of theirs can carry them
    for c in R.CASES:
        if R.kernel_of(c.label) not in ("kq", "g64_bk16", "g64_bk64"):
            assert not c.cmul and not c.asum and c.scn == 1 and not c.ccol, c.name
    # empty last slabs, all four orientations on the strided kernels, misaligned operands, batch gaps, deferred slabs
    assert any(c.nsplit > 1 and (c.nsplit - 1) * R._general_path(R.abi(c))[1] >= c.K for c in by["g64_bk16"])
    assert any(c.nsplit > 1 and (c.nsplit - 1) * R._general_path(R.abi(c))[1] >= c.K for c in by["kq"])
    for p in ("kq", "g64_bk64"):
        assert {c.orient for c in by[p]} == {"NN", "NT", "TN", "TT"}, p
        assert any(c.misalign for c in by[p]), p
    assert any(c.nbatch == 3 and c.gap for c in by["kq"]) and any(c.ccol for c in by["kq"])
    for p in ("kq", "g64_bk64", "tile64", "big"):        # one A for all batch entries, column blocks of one C (ops.linear_pair)
        assert any(c.pair for c in by[p]), p
    assert {R.kernel_of(c.label) for c in R.CASES if c.accumulate == 2} >= {"g64_bk16", "kq", "tile64", "big_slabs"}
    labels = [label for _, label, _ in R.GROUPS]
    assert labels.count("group") >= 2 and labels.count("fallback") >= 4
    assert max(len(cs) for _, label, cs in R.GROUPS if label == "group") == R.GROUP_MAX
    assert any(len(cs) == R.GROUP_MAX + 1 for _, label, cs in R.GROUPS if label == "fallback")
    for _, label, cs in R.GROUPS:
        if label == "group" and len(cs) == R.GROUP_MAX:   # different tile counts: the smaller products' workgroups return early
            assert len({(R.cdiv(c.M, 32), R.cdiv(c.N, 32)) for c in cs}) >= 5


def test_no_case_is_skipped():
    for c in ALL_ENTRIES + R.REFUSALS:
        assert isinstance(c, R.Case)                      # (no pytest.param with marks in the tables)
    for f in ("gemm_ref.py", "test_gemm_kernels_gpu.py"):
        text = open(os.path.join(ROOT, "tests", f)).read()
        for word in ("sk" + "ip", "xf" + "ail", "import" + "orskip"):
            assert word not in text, (f, word)


def test_workspace_formula_is_what_ops_mm_allocates(monkeypatch):
    asked = []

    def scratch(device, n):
        asked.append(n)
        return torch.empty(1)

    monkeypatch.setattr(ops, "scratch", scratch)
    monkeypatch.setattr(ops, "_chk", lambda t, nd=None: t)
    monkeypatch.setattr(ops.hip, "call", lambda *a: None)
    for M, N, K, nsplit, asum in ((40, 100, 300, 3, True), (40, 100, 300, 3, False), (512, 512, 256, 4, False), (70, 33, 300, 4, True)):
        del asked[:]
        ops.mm(torch.empty(M, K), torch.empty(K, N), torch.empty(M, N), nsplit=nsplit, asum=torch.empty(M) if asum else None)
        assert asked == [R.ws_floats(M, N, 1, nsplit, asum)]
        assert R.Layout(R.Case("ws", "kq", M, N, K, nsplit=nsplit, asum=asum)).ws_need == asked[0]
