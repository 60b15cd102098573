"""Device ratios of the single-launch collapsed bound (and of the multi-launch forms) against the long-double reference
tests/vfe_reference.py: per cell and output group the worst |device - reference| / condition scale, beside the float64 level e64 the
tolerance of tests/test_small_reference_gpu.py is made of (tolerance = 10 max(e64, 1e-13)).

    python tools/small_reference_ratios.py [--out profiles/small_reference_ratios.json]       # on the GPU

It runs the test file's own cell runners without their tolerance assertions (every other check of theirs stays: info == 0, bit-equal
repeats), so a cell over its tolerance is reported, not hidden; any other error ends the run at that cell.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_reference_ratios.json"))
    args = ap.parse_args()
    import ggp_amd
    import test_small_reference_gpu as T
    import vfe_reference as V
    engine = ggp_amd.HipEngine()
    cells = {}

    def record(name, w, e64):
        cells[name] = {k: {"ratio": float("%.2g" % w[k]), "e64": e64[k], "tolerance": V.tolerance(e64[k])} for k in w}

    for name in T.SINGLE:
        record(name, T.run_cell(engine, name, strict=False), T.E64[name])
    record("65-17-2-rbf-strided", T.run_strided(engine, strict=False), T.E64["65-17-2-rbf"])
    for name, w in T.run_batch(engine, strict=False).items():
        record(name, w, T.E64[name])
    for name in V.MULTI:
        for form in ("whitened", "streaming"):
            record("%s %s" % (name, form), T.run_multi(engine, name, form, strict=False), T.E64[name] if form == "whitened" else T.E64_STREAM[name])
    worst = {}
    for which, pick in (("single_launch", lambda n: " " not in n), ("multi_launch_whitened", lambda n: n.endswith(" whitened")),
                        ("multi_launch_streaming", lambda n: n.endswith(" streaming"))):
        groups = {}
        for n, c in cells.items():
            if pick(n):
                for k, v in c.items():
                    g = groups.setdefault(k, {"ratio": 0.0, "e64": 0.0, "ratio_over_tolerance": 0.0})
                    g["ratio"], g["e64"] = max(g["ratio"], v["ratio"]), max(g["e64"], v["e64"])
                    g["ratio_over_tolerance"] = max(g["ratio_over_tolerance"], float("%.2g" % (v["ratio"] / v["tolerance"])))
        worst[which] = groups
    import torch
    prop = torch.cuda.get_device_properties(engine.device)
    doc = {"device": {"name": prop.name, "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count}, "rule": "|got - ref| <= 10 max(e64, 1e-13) scale, component-wise",
           "worst_per_group": worst, "cells": cells}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(worst, indent=1))


if __name__ == "__main__":
    main()
