"""SGPMC rates: ms per ``SgpmcTarget.logp_and_grad`` beside ms per ``CollapsedBound(form="whitened").value_and_grad`` at the same shape
and theta (the second is existing code: the yardstick), and transitions/s of ``sample_hmc`` at the two small shapes.

One process; warm-up first; the device is synchronised around every timed block; the two sides ALTERNATE (a, b, a, b, ...) so that
clock drift hits both alike; at least ``--reps`` repetitions and one second per cell; median, quartiles and extremes are recorded.

    python tools/sgpmc_rates.py [--reps 20] [--shapes c1,elevator,c3,c5] [--out profiles/sgpmc_rates.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggp_amd  # noqa: E402

SHAPES = {"c1": ("C1-like", 500, 1, 50), "elevator": ("Elevator-like", 13279, 18, 100), "c3": ("C3", 13279, 18, 512),
          "c5": ("C5", 1_000_000, 8, 1024)}
JITTER = 1e-5
TAIL_LAUNCHES = 4   # csrc/sgp_sgpmc.hip with the adjoints: mid kernel, two gemm() calls, closing kernel


def problem(N, d, M, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    w = rng.standard_normal(d) / math.sqrt(d)
    y = np.sin(2.0 * X @ w) + 0.1 * rng.standard_normal(N)
    y = (y - y.mean()) / y.std()
    return X, y, X[rng.choice(N, M, replace=False)].copy()


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median": round(statistics.median(ms), 4), "q1": round(q[0], 4), "q3": round(q[2], 4), "min": round(min(ms), 4),
            "max": round(max(ms), 4), "reps": len(ms)}


def alternate(fa, fb, reps, min_seconds=1.0, warm=3):
    for _ in range(warm):
        fa(), fb()
    ta, tb = [], []
    t_start = time.perf_counter()
    while len(ta) < reps or time.perf_counter() - t_start < min_seconds:
        for fn, acc in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3)
    return ta, tb


def count_launches(fn):
    """Kernel launches of one call, from the profiler's device activity (None where the profiler does not report them)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if getattr(ev, "device_type", None) is not None and "cuda" in str(ev.device_type).lower()
                and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower())
        return n or None
    except Exception:  # noqa: BLE001 - a measurement aid: absent is "not measured"
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="c1,elevator,c3,c5")
    ap.add_argument("--out", default="profiles/sgpmc_rates.json")
    ap.add_argument("--no-launch-count", action="store_true")
    a = ap.parse_args()
    eng = ggp_amd.HipEngine()
    D = lambda t: torch.as_tensor(t, dtype=torch.float64, device=eng.device).contiguous()
    sp_inv = lambda c: c + math.log(-math.expm1(-c))
    rows = []
    for key in a.shapes.split(","):
        name, N, d, M = SHAPES[key]
        X, y, Z = problem(N, d, M)
        Xd, yd, Zd = D(X), D(y), D(Z)
        ls, sf2, s2 = [math.sqrt(d) * 1.2] * d, 1.0, 0.1
        tgt = ggp_amd.SgpmcTarget(Xd, yd, Zd, jitter=JITTER, engine=eng)
        cb = ggp_amd.CollapsedBound(Xd, yd, jitter=JITTER, engine=eng, form="whitened")
        rng = np.random.default_rng(1)
        q = np.array([sp_inv(sf2)] + [sp_inv(v) for v in ls] + [sp_inv(s2 - 1e-6)] + list(0.5 * rng.standard_normal(M)))
        fa = lambda: tgt.logp_and_grad(q)
        fb = lambda: cb.value_and_grad(Zd, ls, sf2, s2)
        lp, _ = fa()
        F, g = fb()
        assert math.isfinite(lp) and math.isfinite(F), (lp, F)
        ta, tb = alternate(fa, fb, a.reps)
        row = {"shape": name, "N": N, "d": d, "M": M, "pass1": tgt.last_pass1, "ms_sgpmc_logp_and_grad": spread(ta),
               "ms_collapsed_whitened_value_and_grad": spread(tb), "collapsed_single_launch": bool(cb._small_ok(M)),
               "ratio_sgpmc_over_collapsed": round(statistics.median(ta) / statistics.median(tb), 4),
               "tail_launches": TAIL_LAUNCHES,
               "launches_per_sgpmc_evaluation": None if a.no_launch_count else count_launches(fa)}
        if cb._small_ok(M):   # like for like at the small shapes: the collapsed bound through its multi-launch whitened path as well
            cb.fused = False
            ta2, tb2 = alternate(fa, fb, a.reps)
            row["ms_collapsed_whitened_multi_launch"] = spread(tb2)
            row["ms_sgpmc_beside_multi_launch"] = spread(ta2)
            if not a.no_launch_count:
                row["launches_per_collapsed_multi_launch_evaluation"] = count_launches(fb)
        if key in ("c1", "elevator"):
            n_tr = 40
            t0 = time.perf_counter()
            tr = ggp_amd.sample_hmc(tgt, n_tr, 0, seed=3, start=q)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            row["sample_hmc_transitions_per_s"] = round(n_tr / wall, 2)
            row["sample_hmc_leapfrogs_per_transition"] = 10
            row["sample_hmc_seconds_per_1000_draws"] = round(1000.0 * wall / n_tr, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del tgt, cb, Xd, yd, Zd
        eng._ws.clear()
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "reps_min": a.reps, "rates": rows,
           "reference_sampler_runtime_s_per_run": [29, 89]}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
