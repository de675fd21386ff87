"""Bit fingerprint of the step engines: for every configuration of tests/step_helpers.py, three steps on fixed seeds (as a HIP graph
where the engine has that form; --eager for the other), then one line per tensor the steps leave behind -- SHA-256 of each trained
net's flat parameters and gradients, of its Adam m, v and state, of every buffer and seed counter of every net -- and the losses of
every step as hex floats.  Behind the configurations, the paths of the nets that no step runs, because a step's fused loss launch
replaces them: for UpperNet, UpperNetwlocal and LowerNet on the same minibatch the public forward in eval mode (the Upper nets) and in
train mode through autograd with `l.sum().backward()` behind it, once with the differentiable inputs requiring grad and once without
-- outputs, input gradients, the flat gradient buffer and every buffer.

For a one-off A/B of two trees on one device with one built library: the `mmego_amd` package is taken from PYTHONPATH when it is
there (the other tree), from this tree otherwise; the configurations always come from this tree's tests/step_helpers.py.

    MMEGO_HIP_LIB=<library> PYTHONPATH=<other tree> python scripts/step_fingerprint.py > a.txt
    MMEGO_HIP_LIB=<library> python scripts/step_fingerprint.py > b.txt && cmp a.txt b.txt

The hashes belong to one device and one library build: compare them, do not commit them."""
import os
import sys

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


def main():
    import mmego_amd
    print("package:", os.path.dirname(os.path.abspath(mmego_amd.__file__)), file=sys.stderr)
    dev = torch.device("cuda:0")
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


if __name__ == "__main__":
    main()
