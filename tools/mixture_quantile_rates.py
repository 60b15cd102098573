"""Rates of the mixture quantiles (sgp_mixture_quantiles) beside the launches that feed them (sgp_exact_predict_batch +
sgp_exact_mixture_reduce) and beside the host route the library offered before (``get_posterior_predictive_uncertainty_intervals`` per
data set on the copied moments), at (B data sets, S draws, T test points) = (1, 256, 100), (256, 256, 500), (256, 4096, 500) and Q = 2
probabilities (2.5 % and 97.5 %).

    python tools/mixture_quantile_rates.py [--rounds 7] [--out profiles/mixture_quantile_rates.json]

The moments are those of the exact predictive of one data set (N = 32, d = 1) at B x S hyper-parameter rows over the range a posterior
covers.  The two device stages are timed in interleaved rounds in one process (HIP events around the launches alone, three warm-up
rounds), median and minimum over --rounds.  ``iters``: the passes per point the kernel reports.  The host route is timed (wall clock,
two runs, the faster) at the first cell only and extrapolated per (draw x test point x probability) to the others.  Every cell is a child
process of its own under a time limit (--cell I is what the child runs); the first step that fails ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELLS = ((1, 256, 100), (256, 256, 500), (256, 4096, 500))   # (B, S, T)
PROBS = (0.025, 0.975)
N, D = 32, 1
STEP_LIMIT_S = 420


def cell(shape, rounds, host_route):
    import torch
    import ggp_amd
    B, S, T = shape
    P = B * S
    rng = np.random.default_rng(0)
    X = np.sort(rng.uniform(0.0, 10.0, (N, D)), 0)
    y = np.sin(X[:, 0]) + 0.2 * rng.standard_normal(N)
    Xs = rng.uniform(0.0, 10.0, (T, D))
    theta = np.exp(np.concatenate([rng.uniform(np.log(0.7), np.log(2.0), (P, D)), rng.uniform(np.log(0.5), np.log(2.0), (P, 1)),
                                   rng.uniform(np.log(0.02), np.log(0.2), (P, 1))], 1))
    eng = ggp_amd.HipEngine()
    T_ = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)  # noqa: E731
    Xd, yd, Xsd, thd = T_(X), T_(y), T_(Xs), T_(theta)
    Yt = T_(np.sin(Xs[:, 0])[None] + 0.2 * rng.standard_normal((B, T)))
    off = [b * S for b in range(B + 1)]
    state = {}

    def feed():   # the launches that produce the moments and the mixture's two moments and log density
        state["m"], state["v"], state["i"] = eng.exact_predict_batch(Xd, yd, thd, Xsd)
        eng.exact_mixture(state["m"], state["v"], state["i"], off, Ytest=Yt)

    def stage():  # the new stage, on the moments where they are
        state["r"] = eng.mixture_quantiles(state["m"], state["v"], state["i"], off, PROBS, Ytest=Yt, want_iters=True)

    def ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    for _ in range(3):
        feed(), stage()
    torch.cuda.synchronize()
    t_feed, t_stage = [], []
    for _ in range(rounds):   # interleaved: both see the same clocks and the same neighbours
        t_feed.append(ms(feed)), t_stage.append(ms(stage))
    r = state["r"]
    assert int((state["i"] != 0).sum()) == 0 and bool(r["quantiles"].isfinite().all()) and bool(r["pit"].isfinite().all())
    iters = r["iters"].to(torch.float64)
    work = P * T * len(PROBS)
    row = {"B": B, "S": S, "T": T, "Q": len(PROBS), "rounds": rounds,
           "quantiles_ms_median": round(statistics.median(t_stage), 4), "quantiles_ms_min": round(min(t_stage), 4),
           "quantiles_us_per_draw_point_prob": round(1e3 * statistics.median(t_stage) / work, 7),
           "iters_per_point_mean": round(float(iters.mean()), 2), "iters_per_point_max": int(iters.max()),
           "predictive_and_mixture_ms_median": round(statistics.median(t_feed), 4), "predictive_and_mixture_ms_min": round(min(t_feed), 4),
           "quantiles_over_predictive": round(statistics.median(t_stage) / statistics.median(t_feed), 3)}
    if host_route:
        mean, sd = state["m"].cpu().numpy().reshape(B, S, T), np.sqrt(state["v"].cpu().numpy().reshape(B, S, T))
        secs = []
        for _ in range(2):
            t0 = time.perf_counter()
            out = [ggp_amd.get_posterior_predictive_uncertainty_intervals(mean[b], sd[b]) for b in range(B)]
            secs.append(time.perf_counter() - t0)
        lo = np.stack([o[0] for o in out])
        assert np.allclose(lo, r["quantiles"][:, 0].cpu().numpy(), rtol=1e-9, atol=1e-9)
        row.update(host_route_ms=round(1e3 * min(secs), 1), host_route_us_per_draw_point_prob=round(1e6 * min(secs) / work, 5))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="profiles/mixture_quantile_rates.json")
    ap.add_argument("--cell", type=int, default=-1, help="(internal) run cell number I in this process and print its JSON line")
    a = ap.parse_args()
    if a.cell >= 0:
        print("RESULT " + json.dumps(cell(CELLS[a.cell], a.rounds, host_route=a.cell == 0)), flush=True)
        return
    rows = []
    for i, shape in enumerate(CELLS):
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--cell", str(i),
                            "--rounds", str(a.rounds)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-4000:])
            raise SystemExit("step %s ended with status %d: nothing more is started on the GPU" % (shape, r.returncode))
        rows.append(json.loads(line[0][len("RESULT "):]))
        print(json.dumps(rows[-1]), flush=True)
    per = rows[0]["host_route_us_per_draw_point_prob"]
    for row in rows[1:]:   # the host route costs the same per (draw x point x probability) whatever the shape: extrapolated
        work = row["B"] * row["S"] * row["T"] * row["Q"]
        row["host_route_ms_extrapolated"] = round(1e-3 * per * work, 1)
    for row in rows:
        host = row.get("host_route_ms", row.get("host_route_ms_extrapolated"))
        row["host_over_quantiles"] = round(host / row["quantiles_ms_median"], 1)
    import torch
    res = {"device": torch.cuda.get_device_name(0), "probs": list(PROBS), "N": N, "d": D, "cells": rows}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
