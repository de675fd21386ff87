"""The BiLSTM(64) recurrence kernels (lstm64_fwd / lstm64_bwd and their _multi forms) in a kernel trace and in counter passes, per
instantiation: launches, grid, average / min / max us from a `rocprofv3 --kernel-trace` database, and per-launch averages of whatever
counters `rocprofv3 --pmc ... --output-format csv` passes collected (runs of their own, never with tracing).

usage: python scripts/lstm64_profile_summary.py LABEL=trace.db[,pmc_dir] [LABEL=...] > profiles/<name>.json
  trace:    rocprofv3 --kernel-trace -d DIR -o bench -- python3 bench.py --steps 6 --warmup 2 --trace-only --sequential
  counters: rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d DIR -o pmc --
            python3 bench.py --steps 4 --warmup 2 --trace-only --no-graph"""
import collections
import csv
import glob
import json
import os
import re
import sqlite3
import sys

short = lambda n: re.sub(r"\(.*", "", n).replace("void ", "")
out = {}
for arg in sys.argv[1:]:
    label, _, paths = arg.partition("=")
    db, _, pmc = paths.partition(",")
    res = out[label] = {"trace": {}, "counters_avg_per_launch": {}}
    by = collections.defaultdict(list)
    for n, gx, wx, s, e in sqlite3.connect(db).execute("select name, grid_x, workgroup_x, start, end from kernels order by start"):
        if "lstm64" in n:
            by[(short(n), gx // max(wx, 1))].append((e - s) / 1e3)
    for (n, wgs), v in sorted(by.items()):
        res["trace"][n] = {"workgroups_x": wgs, "launches": len(v), "avg_us": round(sum(v) / len(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    fam = collections.defaultdict(list)
    for (n, _), v in by.items():
        fam[n.split("<")[0]] += v
    res["trace_by_family_avg_us"] = {n: round(sum(v) / len(v), 2) for n, v in sorted(fam.items())}
    if pmc:
        c = collections.defaultdict(lambda: collections.defaultdict(list))
        for f in glob.glob(os.path.join(pmc, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "lstm64" in r["Kernel_Name"]:
                    c[short(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
        for n, cs in sorted(c.items()):
            res["counters_avg_per_launch"][n] = dict({k: round(sum(v) / len(v), 1) for k, v in sorted(cs.items())}, launches=len(next(iter(cs.values()))))
print(json.dumps(out, indent=1))
