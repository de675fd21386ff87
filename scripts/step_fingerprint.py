"""Bit fingerprint of the step engines: for every configuration of tests/step_helpers.py, three steps on fixed seeds (as a HIP graph
where the engine has that form; --eager for the other), then one line per tensor the steps leave behind -- SHA-256 of each trained
net's flat parameters and gradients, of its Adam m, v and state, of every buffer and seed counter of every net -- and the losses of
every step as hex floats.

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


if __name__ == "__main__":
    main()
