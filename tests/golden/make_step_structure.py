"""Writes tests/golden/step_structure.json: the launch structure of one whole step() of every step engine of mmego_amd/train_step.py
(StageStep in its ten forms, ImuStep with and without dropout, ConcurrentStages as branches and as one chain, SharedImuStages,
PipelinedStages in fp32 and split3), which tests/test_step_engines_gpu.py::test_step_structure_is_the_recorded_one holds every later
commit to.  The configurations and what is dumped: tests/step_helpers.py.

The file is a record of what the code did BEFORE a change that must not move a launch.  To regenerate it, check out the commit whose
structure is to be kept (with this script and tests/step_helpers.py beside it), build the library, and on the GPU run

    python tests/golden/make_step_structure.py

Regenerating it on the commit under test makes the test say nothing."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import step_helpers as sh  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    out = {}
    for name in sh.CONFIGS:
        eng, _ = sh.build(name, dev, use_graph=False)
        out[name] = sh.step_structure(eng)
        print("%-26s %d segments, %d launches" % (name, len(out[name]["segments"]), sum(len(s["calls"]) for s in out[name]["segments"])))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "step_structure.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
