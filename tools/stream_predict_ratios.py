"""Device ratios of the streaming posterior predictive (sgp_predict from the factors of either form of CollapsedBound,
sgp_mixture_predict, sgp_mixture_predict_zs) against the long-double reference tests/vfe_predict_reference.py: per cell, route and
output the worst |device - reference| / condition scale beside the tolerance 10 max(e64, 1e-13) of tests/test_stream_predict_gpu.py.

    python tools/stream_predict_ratios.py [--out profiles/stream_predict_anchor.json]       # on the GPU

It runs the test files' own check functions without their tolerance assertions (every other check of theirs stays: info == 0, the caps on
the tolerance, symmetric covariances, bit-equal repeats), so a cell over its tolerance is reported, not hidden; any other error ends the
run at that cell.  Written as cell -> route -> output -> [worst, tolerance]; a mixture route reports the draw closest to its tolerance.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_predict_anchor.json"))
    args = ap.parse_args()
    import torch

    import ggp_amd
    import test_stream_predict as T
    import vfe_predict_reference as R
    from conftest import dev
    engine = ggp_amd.HipEngine()
    conv = lambda a: dev(a, engine)  # noqa: E731
    cells = {}

    def record(name, routes):
        for route, w in routes.items():
            cells.setdefault(name, {})[route] = {k: [float("%.2g" % v[0]), float("%.2g" % v[1])] for k, v in w.items()}

    for form in R.ROUTES:
        for name in R.stream_cells(form):
            record(name, T.check_predict_cell(engine, conv, name, form, strict=False))
        record(R.BIG_T_CELL, T.check_predict_big_t(engine, conv, form, bits=True, strict=False))
    for name in R.STREAM_STATIONARY:
        record(name, T.check_mixture_cell(engine, conv, name, strict=False))
    record(T.ZS_CELL, T.check_mixture_cell(engine, conv, T.ZS_CELL, zs=True, strict=False))
    record(R.BIG_T_CELL, {"mixture_T%d" % R.BIG_T[0]: T.check_mixture_cell(engine, conv, R.BIG_T_CELL, T=R.BIG_T[0], strict=False)["mixture"]})
    worst = {}
    for name, routes in cells.items():
        for route, w in routes.items():
            kind = route.split("_T")[0]
            for k, (v, tol) in w.items():
                g = worst.setdefault(kind, {}).setdefault(k, {"ratio": 0.0, "ratio_over_tolerance": 0.0, "closest_to_tolerance_at": ""})
                g["ratio"] = max(g["ratio"], v)
                if v / tol > g["ratio_over_tolerance"]:
                    g["ratio_over_tolerance"], g["closest_to_tolerance_at"] = float("%.2g" % (v / tol)), name
    prop = torch.cuda.get_device_properties(engine.device)
    doc = {"device": {"name": prop.name, "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count},
           "rule": "|got - ref| <= 10 max(e64, 1e-13) scale, component-wise; entries are [worst |got - ref| / scale, tolerance]",
           "worst_per_route": worst, "cells": cells}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(worst, indent=1))


if __name__ == "__main__":
    main()
