"""GPU: mmego_gemm and mmego_gemm_group (csrc/gemm.hip, csrc/gemm_tile.hip) through the C ABI with raw strides, on every kernel the
launcher can choose and with every option it accepts there, against the float64 restatement of the contract in tests/gemm_ref.py.

Per case (gemm_ref.CASES: the smallest shapes that reach each path) two data sets: small integers, where every kernel has to return
the float64 result EXACTLY whatever its summation order, and unit normals against the a-priori bound of gemm_ref.bound() times 1.001
-- no measured margin.  Every output buffer is wider than the contract and pre-filled with one NaN bit pattern that must survive
bit for bit outside the elements the contract writes (between strided rows and columns, between batch entries, behind the documented
workspace size, all of C in the deferred form); inputs are surrounded by NaN and must come back unchanged.  The table's label of a
case has to be what gemm_ref.path_of() derives from the launcher's rules; tests/test_gemm_ref_cpu.py checks the reference, the bound
and the table's coverage without a GPU."""
import ctypes

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

DEVICE_REF_FROM = 1 << 20          # outputs from which the float64 reference is computed on the device, not on the host


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def prepare(dev, c, kind):
    """-> (device buffers, their state before the call, reference, bound or None)."""
    bufs = R.make_bufs(c, kind, device=dev)
    pre = {k: v.clone() for k, v in bufs.items() if v is not None}
    src = pre if c.M * c.N * c.nbatch >= DEVICE_REF_FROM else {k: v.cpu() for k, v in pre.items()}
    src = dict({k: None for k in bufs}, **src)
    return bufs, pre, R.ref(c, src), R.bound(c, src) if kind == "normal" else None


def worst(err, tol):
    """(b, m) or (b, m, n) of the element furthest outside its tolerance (NaN counts as furthest), and its figures."""
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / tol.clamp_min(1e-300))
    i = int(ratio.argmax())
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), err.shape))
    return idx, float(err.flatten()[i]), float(tol.flatten()[i])


def compare(c, kind, what, got, want, bnd):
    got = got.double().to(want.device)
    tag = "%s [%s] %s data, %s" % (c.name, R.path_of(c), kind, what)
    if kind == "int":
        if not torch.equal(got, want):
            idx, e, _ = worst((got - want).abs(), torch.ones_like(want))
            raise AssertionError("%s: not exact; worst at (b, m, n) = %s: |out - ref| = %g, %d elements differ"
                                 % (tag, idx, e, int((got != want).sum())))
    else:
        err, tol = (got - want).abs(), R.SECOND_ORDER * bnd
        if not bool((err <= tol).all()):
            idx, e, t = worst(err, tol)
            raise AssertionError("%s: outside the bound; worst at (b, m, n) = %s: |out - ref| = %g > %g" % (tag, idx, e, t))


def check_untouched(c, bufs, pre, written=None):
    """Everything outside the contract's writes is bit-identical to its state before the call; inputs entirely."""
    written = written if written is not None else R.written_mask(c, bufs)
    for name, before in pre.items():
        a, b = bufs[name].view(torch.int32), before.view(torch.int32)
        diff = a != b
        if name in written:
            diff &= ~written[name]
        if bool(diff.any()):
            i = int(diff.nonzero()[0])
            raise AssertionError("%s [%s]: %s was written outside the contract at float %d (of %d): 0x%08x -> 0x%08x"
                                 % (c.name, R.path_of(c), name, i, a.numel(), int(b[i]) & 0xFFFFFFFF, int(a[i]) & 0xFFFFFFFF))


def check_results(c, kind, bufs, pre, want, bnd):
    check_untouched(c, bufs, pre)
    v = R.views(c, bufs)
    pick = lambda k: None if bnd is None else bnd[k]
    if c.accumulate != 2:
        compare(c, kind, "C", v["C"], want["C"], pick("C"))
        if c.asum:
            compare(c, kind, "asum", v["asum"][..., None], want["asum"][..., None], None if bnd is None else bnd["asum"][..., None])
        return
    # deferred: the float64 sum of the slabs is the product; the slab row sums sit behind the slabs
    n = c.nsplit * c.nbatch * c.M * c.N
    slabs = bufs["ws"][:n].view(c.nsplit, c.nbatch, c.M, c.N).double().sum(0)
    compare(c, kind, "sum of the deferred slabs", slabs, want["prod"], pick("prod"))
    if c.asum:
        rows = bufs["ws"][n:n + c.nsplit * c.nbatch * c.M].view(c.nsplit, c.nbatch, c.M, 1).double().sum(0)
        compare(c, kind, "sum of the deferred slab row sums", rows, want["asum"][..., None], None if bnd is None else bnd["asum"][..., None])


def launch(c, bufs):
    from mmego_amd import hip
    hip.call("gemm", *R.abi(c, bufs).values())


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_gemm_case(dev, c):
    assert R.path_of(c) == c.label, "%s: the table says %s, the launcher's rules say %s" % (c.name, c.label, R.path_of(c))
    for kind in ("int", "normal"):
        bufs, pre, want, bnd = prepare(dev, c, kind)
        launch(c, bufs)
        torch.cuda.synchronize()
        check_results(c, kind, bufs, pre, want, bnd)


@pytest.mark.parametrize("c", R.REFUSALS, ids=lambda c: c.name)
def test_gemm_refusal(dev, c):
    assert R.path_of(c) == "refused"
    bufs = R.make_bufs(c, "int", device=dev)
    pre = {k: v.clone() for k, v in bufs.items() if v is not None}
    with pytest.raises(RuntimeError, match="mmego_gemm failed: bad argument"):
        launch(c, bufs)
    torch.cuda.synchronize()
    check_untouched(c, bufs, pre, written={})


def launch_group(cases, all_bufs):
    from mmego_amd import hip
    arr = (hip.GemmDesc * len(cases))()
    for dsc, c, bufs in zip(arr, cases, all_bufs):
        for name, value in R.abi(c, bufs).items():
            setattr(dsc, name, hip._conv(value))
    assert ctypes.sizeof(arr) == len(cases) * ctypes.sizeof(hip.GemmDesc)
    hip.call("gemm_group", len(cases), arr)


@pytest.mark.parametrize("name,label,cases", R.GROUPS, ids=[g[0] for g in R.GROUPS])
def test_gemm_group(dev, name, label, cases):
    assert R.group_path_of(cases) == label, "%s: the table says %s, the launcher's rules say %s" % (name, label, R.group_path_of(cases))
    for kind in ("int", "normal"):
        prepared = [prepare(dev, c, kind) for c in cases]
        launch_group(cases, [p[0] for p in prepared])
        torch.cuda.synchronize()
        for c, (bufs, pre, want, bnd) in zip(cases, prepared):
            assert R.path_of(c) == c.label, (name, c.name)
            check_results(c, kind, bufs, pre, want, bnd)


@pytest.mark.parametrize("name,cases", R.GROUP_REFUSALS, ids=[g[0] for g in R.GROUP_REFUSALS])
def test_gemm_group_refusal(dev, name, cases):
    assert R.group_path_of(cases) == "refused"
    all_bufs = [R.make_bufs(c, "int", device=dev) for c in cases]
    pre = [{k: v.clone() for k, v in bufs.items() if v is not None} for bufs in all_bufs]
    with pytest.raises(RuntimeError, match="mmego_gemm_group failed: bad argument"):
        launch_group(cases, all_bufs)
    torch.cuda.synchronize()
    for c, bufs, p in zip(cases, all_bufs, pre):          # no entry has run, the acceptable ones in front of the refused one included
        check_untouched(c, bufs, p, written={})


def test_group_of_nothing_is_refused(dev):
    from mmego_amd import hip
    with pytest.raises(RuntimeError, match="bad argument"):
        hip.call("gemm_group", 0, (hip.GemmDesc * 1)())
    with pytest.raises(RuntimeError, match="bad argument"):
        hip.call("gemm_group", 2, None)


def test_device_reference_is_the_host_reference(dev):
    """The larger cases' float64 references are computed on the device: the same numbers as on the host."""
    c = next(x for x in R.CASES if x.name == "tile64_split4_reduce")
    bufs = R.make_bufs(c, "normal", device=dev)
    host = {k: (v.cpu() if v is not None else None) for k, v in bufs.items()}
    on_dev, on_host, bnd = R.ref(c, bufs)["C"].cpu(), R.ref(c, host)["C"], R.bound(c, host)["C"]
    assert bool(((on_dev - on_host).abs() <= 1e-6 * bnd).all())
    assert bool(((R.bound(c, bufs)["C"].cpu() - bnd).abs() <= 1e-6 * bnd).all())
