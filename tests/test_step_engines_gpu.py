"""GPU: the step engines of mmego_amd/train_step.py as a whole -- what a step() launches and in which order on which streams
(against tests/golden/step_structure.json), graph replay against the eager body bit for bit, and the optimisers a trainer hands to
every step it builds."""
import json
import os

import pytest
import torch

import step_helpers as sh
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from mmego_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def test_step_structure_is_the_recorded_one(dev):
    """One whole eager step() of every one of the 17 configurations of tests/step_helpers.py -- body, all-reduce, optimisers -- recorded with
    plan.StepPlan: segments, their streams, what each waits for, every entry point in order and the final waits equal
    tests/golden/step_structure.json, which tests/golden/make_step_structure.py wrote on the commit BEFORE the engines were moved onto
    one capture protocol and one table of trained nets (the three configurations added since -- upper_wlocal_finetune_imu,
    lower_frozen_wlocal, lower_finetune_all -- on the commit before the two Upper nets got one base class).  No tolerance, nothing left
    out."""
    want = json.load(open(os.path.join(GOLDEN, "step_structure.json")))
    assert sorted(want) == sorted(sh.CONFIGS)
    bad = []
    for name in sh.CONFIGS:
        eng, _ = sh.build(name, dev, use_graph=False)
        diff = sh.first_difference(name, sh.step_structure(eng), want[name])
        if diff is not None:
            print(diff)
            bad.append(diff)
    assert not bad, bad


def test_every_launch_of_a_step_matches_its_declaration(dev):
    """One whole step() of every one of the 17 configurations, recorded with plan.StepPlan: every (entry point, arguments) has as many arguments, with the
    stream, as include/mmego_hip.h declares parameters, and every argument sits on a parameter of its kind -- a tensor, None, ctypes
    array or Structure on a pointer; a Python float on a float or double; a bool or int (a raw address is an int) on an int, a long or
    a pointer.  ctypes itself accepts surplus trailing arguments, and a tensor becomes an integer that a long parameter would swallow."""
    import ctypes
    from mmego_amd import hip
    from mmego_amd.plan import StepPlan
    protos = hip.parse_header()
    kinds = (((torch.Tensor, type(None), ctypes.Array, ctypes.Structure), (ctypes.c_void_p,)),
             ((float,), (ctypes.c_float, ctypes.c_double)),
             ((bool, int), (ctypes.c_int, ctypes.c_long, ctypes.c_void_p)))
    bad, nlaunch = [], 0
    for name in sh.CONFIGS:
        eng, _ = sh.build(name, dev, use_graph=False)
        eng.step()
        torch.cuda.synchronize()
        for sg in StepPlan().record(eng.step).segments:
            for entry, args in sg.calls:
                nlaunch += 1
                (stream_t, stream_name), params = protos["mmego_" + entry][0], protos["mmego_" + entry][1:]
                assert stream_t is ctypes.c_void_p and stream_name == "stream", entry
                if len(args) != len(params):
                    bad.append("%s: %s takes %d arguments behind the stream, %d given" % (name, entry, len(params), len(args)))
                    continue
                for v, (ct, pname) in zip(args, params):
                    allowed = [cts for pys, cts in kinds if isinstance(v, pys)]
                    if not allowed or ct not in allowed[0]:
                        bad.append("%s: %s(%s): a %s on a %s parameter" % (name, entry, pname, type(v).__name__, ct.__name__))
    print("%d launches checked" % nlaunch)
    assert nlaunch > 17 * 20 and not bad, sorted(set(bad))


@pytest.mark.parametrize("name", ["imu_step_dropout", "upper_finetune_imu", "lower_finetune_upper", "shared_fp32"])
def test_graph_form_equals_eager_form(dev, name):
    """Two steps as a replayed HIP graph and two steps of the eager body, same start (tests/step_helpers.py's shapes): losses, every
    trained net's flat parameters and gradients, its Adam m, v and state, and every buffer (BatchNorm running statistics, step counters)
    and seed counter of every net the engine runs, bit for bit -- the warm-up runs ahead of the capture leave no trace."""
    res = []
    for use_graph in (False, True):
        eng, nets_ = sh.build(name, dev, use_graph)
        start = [sh.raw(net.flat().flat_p) for _, net, _ in sh.trained(eng)]
        seen = []
        for _ in range(2):
            eng.step()
            seen += [("loss", sh.raw(l)) for l in sh.losses(eng)]
        torch.cuda.synchronize()
        assert (eng.graph is not None) == use_graph
        assert all(not torch.equal(p0, sh.raw(net.flat().flat_p)) for p0, (_, net, _) in zip(start, sh.trained(eng))), name    # (trained)
        res.append(seen + [(k, sh.raw(t)) for k, t in sh.state(eng, nets_)])
    assert [k for k, _ in res[0]] == [k for k, _ in res[1]]
    for (k, a), (_, b) in zip(*res):
        assert torch.equal(a, b), (name, k)


def test_one_optimiser_dict_serves_every_step(dev, monkeypatch):
    """Steps of two minibatch sizes (B=2 and B=4, T=4, N=128) built from ONE optimiser dict share the identical optimiser objects, and
    FusedAdam.__init__ runs once per trained net; a trainer (UpperTrainer's step factory, on a bare object) builds its optimiser once,
    for both sizes, and loads the resume state once, where it builds it."""
    import types

    from mmego_amd import nets, params, processors
    from mmego_amd.train_step import ImuStep, StageStep
    built, loaded = [], []
    init, load = params.FusedAdam.__init__, params.FusedAdam.load_state_dict
    monkeypatch.setattr(params.FusedAdam, "__init__", lambda self, flat, *a, **k: (built.append(flat.module), init(self, flat, *a, **k))[1])
    monkeypatch.setattr(params.FusedAdam, "load_state_dict", lambda self, sd: (loaded.append(self), load(self, sd))[1])
    torch.manual_seed(5)
    up, lo, fr = nets.UpperNet().to(dev).train(), nets.LowerNet(64).to(dev).train(), nets.UpperNet().to(dev).train()
    imu = nets.IMUNet(15, 9, 64, 2, True, 0).to(dev).train()
    for make, keys, trained in (
            (lambda o: StageStep("upper", up, imu, finetune_imu=True, optimisers=o), ("imu_opt", "opt"), [imu, up]),
            (lambda o: StageStep("lower", lo, None, upper_frozen=fr, finetune_upper=True, optimisers=o), ("upper_opt", "opt"), [fr, lo])):
        del built[:]
        opts = {}
        a, b = make(opts), make(opts)
        assert sorted(opts) == sorted(keys) and [id(m) for m in built] == [id(m) for m in trained]
        assert all(getattr(a, k) is getattr(b, k) is opts[k] for k in keys)
    del built[:]
    opt = params.FusedAdam(imu.flat(), lr=1e-4, weight_decay=1e-3)
    assert ImuStep(imu, opt=opt).opt is opt and ImuStep(imu, opt=opt).opt is opt and len(built) == 1

    # the trainer: two sizes, one optimiser, one resume load -- and the steps really run on it
    saved = params.FusedAdam(up.flat(), lr=3e-5)
    saved.step()
    tr = processors.UpperTrainer.__new__(processors.UpperTrainer)
    tr.cfg, tr.pg, tr.device, tr.frame_no, tr.learning_rate = types.SimpleNamespace(), None, dev, 4, 3e-5
    tr.model, tr.model_IMU, tr._steps, tr._opts, tr._resume = up, None, {}, {}, {"optimizer": saved.state_dict()}
    del built[:], loaded[:]
    g = torch.Generator().manual_seed(6)
    for B in (2, 4, 2):
        st = tr._step_for(B)
        st.bind(*[torch.randn(*shape, generator=g).to(dev) for shape in ((B, 4, 128, 6), (B, 4, 20, 15), (B, 20, 3), (B, 4, 21, 3))],
                R_gt=torch.linalg.qr(torch.randn(B, 4, 3, 3, generator=g))[0].contiguous().to(dev))
        st.step()
    torch.cuda.synchronize()
    assert len(tr._steps) == 2 and tr._steps[2].opt is tr._steps[4].opt is tr._opts["opt"] and list(tr._opts) == ["opt"]
    assert [id(m) for m in built] == [id(up)] and loaded == [tr._opts["opt"]]
    assert tr._opts["opt"].state[0].item() == saved.state[0].item() + 3          # (the saved step count, then the three steps)


def test_a_dropped_engine_is_freed_at_once(dev):
    """No engine is part of a reference cycle: dropping the last reference frees it, and with it its HIP graph, there and then.  Left to
    the cyclic collector, the graph could be destroyed while some later capture is under way, which HIP refuses."""
    import gc
    import weakref
    gc.collect()
    gc.disable()
    try:
        for name in sh.CONFIGS:
            eng, nets_ = sh.build(name, dev, use_graph=True)
            ref = weakref.ref(eng)
            del eng
            assert ref() is None, name
    finally:
        gc.enable()
