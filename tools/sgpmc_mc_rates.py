"""Rates of SGPMC with the multi-class robust-max likelihood: device ms per value and per value + gradient of
``SgpmcTarget(likelihood="multiclass")`` for C in {3, 10} beside ``SgpmcTarget(likelihood="bernoulli")`` at the same shape, in the same
call -- the Bernoulli path is the yardstick; the ratio is reported, not asserted.

One process; warm-up first; HIP events on the stream around every timed call (the host side of an evaluation -- one device-to-host
copy -- is inside the bracket, as a sampler sees it); the targets ALTERNATE (a, b, c, a, b, c, ...) so that clock drift hits all
alike; median and quartiles are recorded.  Shapes (N, d, M): (500, 1, 50) and (13279, 18, 100).

    python tools/sgpmc_mc_rates.py [--reps 20] [--out profiles/sgpmc_mc_rates.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ggp_amd  # noqa: E402

SHAPES = [(500, 1, 50), (13279, 18, 100)]
CLASSES = (3, 10)
JITTER = 1e-5
# passes over the N x Mp block T per evaluation with gradients
T_READS = {"bernoulli": "rows 1, g 1, two scalings 2 (in place), contraction 1, pass 2 1 = 6 reads, 2 writes",
           "multiclass": "rows 1 (all classes), g 1 (all classes), two scalings 2 (out of place), two contractions 2 (of the scaled "
                         "copies), fold 1, pass 2 1 = 6 reads of T + 2 of the copy, 3 writes"}


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median": round(statistics.median(ms), 4), "q1": round(q[0], 4), "q3": round(q[2], 4), "reps": len(ms)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps, warm=3):
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    acc = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, acc):
            t.append(timed(fn))
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="profiles/sgpmc_mc_rates.json")
    a = ap.parse_args()
    eng = ggp_amd.HipEngine()
    D = lambda t: torch.as_tensor(t, dtype=torch.float64, device=eng.device).contiguous()
    sp_inv = lambda c: c + math.log(-math.expm1(-c))
    out = []
    for N, d, M in SHAPES:
        rng = np.random.default_rng(0)
        X = rng.standard_normal((N, d))
        F = np.sin(2.0 * X @ (rng.standard_normal((d, max(CLASSES))) / math.sqrt(d)))
        Z = X[rng.choice(N, M, replace=False)].copy()
        Xd, Zd = D(X), D(Z)
        ls, sf2 = [math.sqrt(d) * 1.2] * d, 1.0
        theta = [sp_inv(sf2)] + [sp_inv(t) for t in ls]
        names, tg, qs = ["bernoulli"] + ["multiclass_C%d" % c for c in CLASSES], {}, {}
        tg["bernoulli"] = ggp_amd.SgpmcTarget(Xd, D(np.where(F[:, 0] + 0.3 * rng.standard_normal(N) > 0, 1.0, -1.0)), Zd, jitter=JITTER,
                                              engine=eng, likelihood="bernoulli")
        qs["bernoulli"] = np.array(theta + list(0.5 * rng.standard_normal(M)))
        for c in CLASSES:
            y = np.argmax(F[:, :c] + 0.3 * rng.standard_normal((N, c)), 1).astype(np.float64)
            tg["multiclass_C%d" % c] = ggp_amd.SgpmcTarget(Xd, D(y), Zd, jitter=JITTER, engine=eng, likelihood="multiclass", num_classes=c)
            qs["multiclass_C%d" % c] = np.array(theta + list(0.5 * rng.standard_normal(M * c)))
        for n in names:
            lp, g = tg[n].logp_and_grad(qs[n])
            assert math.isfinite(lp) and all(math.isfinite(t) for t in g), (n, lp)
        val = alternate([lambda n=n: tg[n].logp(qs[n]) for n in names], a.reps)
        grd = alternate([lambda n=n: tg[n].logp_and_grad(qs[n]) for n in names], a.reps)
        row = {"N": N, "d": d, "M": M}
        for i, n in enumerate(names):
            row["ms_value_" + n], row["ms_value_and_grad_" + n] = spread(val[i]), spread(grd[i])
            if i:
                row["ratio_value_%s_over_bernoulli" % n] = round(statistics.median(val[i]) / statistics.median(val[0]), 4)
                row["ratio_value_and_grad_%s_over_bernoulli" % n] = round(statistics.median(grd[i]) / statistics.median(grd[0]), 4)
        out.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "reps": a.reps, "passes_over_T": T_READS, "rates": out}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
