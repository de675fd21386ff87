"""Bit fingerprint of the step engines: for every configuration of tests/step_helpers.py, three steps on fixed seeds (as a HIP graph
where the engine has that form; --eager for the other), then one line per tensor the steps leave behind -- SHA-256 of each trained
net's flat parameters and gradients, of its Adam m, v and state, of every buffer and seed counter of every net -- and the losses of
every step as hex floats.  Behind the configurations, the paths of the nets that no step runs, because a step's fused loss launch
replaces them: for UpperNet, UpperNetwlocal and LowerNet on the same minibatch the public forward in eval mode (the Upper nets) and in
train mode through autograd with `l.sum().backward()` behind it, once with the differentiable inputs requiring grad and once without
-- outputs, input gradients, the flat gradient buffer and every buffer.  Last, the fused Adam step on its own (--adam: this section
alone), where a change that moves all its forms together would pass every test that holds one form to another: each of the eight forms
of csrc/optim.hip (clipped or not, averaged or not, scheduled or not) at 4, 1028 and 2 097 156 floats (one lane; a partial workgroup;
exactly one lane on a second grid-stride trip), weight decay 0 and 1e-3, with two skip ranges of which the second holds the last
float4 (none at 4 floats, where they would leave nothing to update), seven steps on inputs that an integer formula fixes on the host;
step 4's gradient of the clipped forms holds one inf.  The schedule is the step kind of tests/test_lr_schedule_gpu.py, and the cosine
once.  One line per step: SHA-256 of p, m, v, ema, state and stats.

For a one-off A/B of two trees on one device with one built library: the `mmego_amd` package is taken from PYTHONPATH when it is
there (the other tree), from this tree otherwise; the configurations always come from this tree's tests/step_helpers.py.

    MMEGO_HIP_LIB=<library> PYTHONPATH=<other tree> python scripts/step_fingerprint.py > a.txt
    MMEGO_HIP_LIB=<library> python scripts/step_fingerprint.py > b.txt && cmp a.txt b.txt

The hashes belong to one device and one library build: compare them, do not commit them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path += [ROOT, os.path.join(ROOT, "tests")]              # (behind PYTHONPATH: another tree's package wins)

import step_helpers as sh  # noqa: E402


def net_cases(dev):
    from mmego_amd import nets, nets_local
    x, _, body, _, R = sh.batch(dev)
    g = torch.Generator().manual_seed(5)
    t, upper_l = torch.randn(sh.B, sh.T, 3, generator=g).to(dev), torch.randn(sh.B, sh.T, 15, 3, generator=g).to(dev)
    zeros = torch.zeros(6, sh.B, 64, device=dev)
    makes = (("UpperNet", nets.UpperNet, lambda n, u, R, t: n(x.clone(), zeros, zeros, body, R, t), 1),
             ("UpperNetwlocal", nets_local.UpperNetwlocal, lambda n, u, R, t: n(x.clone(), zeros, zeros, zeros, zeros, body, R, t), 2),
             ("LowerNet", lambda: nets.LowerNet(64), lambda n, u, R, t: n(u, x.clone(), None, None, None, None, body, R, t), 0))
    for name, make, call, nattn in makes:
        for case in ("eval", "autograd_inputs", "autograd")[0 if nattn else 1:]:
            torch.manual_seed(1000)
            net = make().to(dev).train(case != "eval")
            if name != "UpperNet":
                net.differentiable_inputs = True
            ins = [v.clone().requires_grad_(case == "autograd_inputs") for v in ((upper_l,) if not nattn else ()) + (R, t)]
            with torch.set_grad_enabled(case != "eval"):
                res = call(net, upper_l if nattn else ins[0], *ins[-2:])
            if case == "eval":
                out = [("l", res[0]), ("q", res[1])] + [("attn%d" % i, res[2 + i]) for i in range(nattn)]
            else:
                res[0].sum().backward()
                out = [("l", res[0])] + [("input%d.grad" % i, v.grad) for i, v in enumerate(ins) if v.grad is not None]
                out += [("flat_g", net.flat().flat_g)] + [("buffer." + k, b) for k, b in net.named_buffers()]
            torch.cuda.synchronize()
            for label, v in out:
                print("net %s %s %s %s" % (name, case, label, sh.sha256(v)))


def fixed(n, salt, scale):
    """n floats in [-scale / 2, scale / 2): the top 24 bits of a multiplicative hash of (index, salt), formed in integers on the host."""
    x = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt * 40503 + 12345)) & np.uint64(0xffffffff)
    x = ((x ^ (x >> np.uint64(15))) * np.uint64(2246822519)) & np.uint64(0xffffffff)
    return torch.from_numpy((((x >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5) * scale).astype(np.float32))


def adam_cases(dev):
    from adam_helpers import AdamSet
    from mmego_amd import hip
    steps, decay = 7, 0.9
    kinds = {"step": hip.LrSchedule(kind=3, warmup=3.0, floor=0.2, every=2.0, gamma=0.5),
             "cosine": hip.LrSchedule(kind=1, warmup=3.0, span=3.0, floor=0.1)}
    forms = [(c, e, s) for c in (False, True) for e in (False, True) for s in (False, True)]
    for n in (4, 1028, 2048 * 256 * 4 + 4):
        p0, grads = fixed(n, 0, 2.0), [fixed(n, k, 0.2) for k in range(1, steps + 1)]
        max_norm = 0.5 * float(grads[0].double().pow(2).sum().sqrt())             # (clipping is live)
        bad = grads[3].clone()
        bad[n - 3] = float("inf")
        grads, bad = [g.to(dev) for g in grads], bad.to(dev)
        skip = torch.tensor([8, 24, n - 8, n], dtype=torch.int64) if n >= 32 else None
        cases = [(form, wd, "step") for form in forms for wd in (0.0, 1e-3)] + ([((True, True, True), 1e-3, "cosine")] if n == 1028 else [])
        for (clipped, averaged, scheduled), wd, kind in cases:
            a = AdamSet(dev, p0, 4 if scheduled else 3)
            opts = dict(decay=decay if averaged else None, max_norm=max_norm if clipped else None, skip=skip)
            for k in range(steps):
                g = bad if clipped and k == 3 else grads[k]
                if scheduled:
                    a.sched_step(g, wd, kinds[kind], **opts)
                else:
                    a.step(g, wd, **opts)
                torch.cuda.synchronize()
                label = "adam%s%s%s" % ("_clipped" * clipped, "_ema" * averaged, ("_sched:" + kind) * scheduled)
                print("%s n=%d wd=%g step %d %s" % (label, n, wd, k + 1, " ".join(
                    "%s %s" % (name, sh.sha256(t)) for name, t in zip(("p", "m", "v", "ema", "stats", "state"), a.tensors() + (a.state,)))))


def main():
    import mmego_amd
    print("package:", os.path.dirname(os.path.abspath(mmego_amd.__file__)), file=sys.stderr)
    dev = torch.device("cuda:0")
    if "--adam" in sys.argv:
        return adam_cases(dev)
    use_graph = "--eager" not in sys.argv
    for name in sh.CONFIGS:
        eng, nets_ = sh.build(name, dev, use_graph)
        for step in range(3):
            eng.step()
            torch.cuda.synchronize()
            print("%s step %d losses %s" % (name, step, " ".join(float(v).hex() for l in sh.losses(eng) for v in l.tolist())))
        for label, t in sh.state(eng, nets_):
            print("%s %s %s" % (name, label, sh.sha256(t)))
    net_cases(dev)
    adam_cases(dev)


if __name__ == "__main__":
    main()
