"""Rates of SGPMC + HMC with a composite kernel at the reference's CO2 shape (N, d, M) = (600, 1, 200):

  * ``CompositeSgpmcTarget.logp_and_grad`` in ms -- median and quartiles, the device synchronised around each call, host work and the
    one device-to-host copy included, after a warm-up;
  * ``CompositeHmcTarget.logp_and_grad`` (the collapsed bound's NUTS target, on its multi-launch path: M = 200 is beyond the
    single-launch code) at the same shape, ALTERNATING with it in the same call -- the one yardstick there is -- and the ratio;
  * launches per evaluation of both, from a profiler pass of its own (torch.profiler's device activity, not timed);
  * ``sample_hmc`` transitions / s at 20 leapfrog steps.

Anything that could not be measured is written "not measured".

    python tools/sgpmc_comp_rates.py [--reps 30] [--transitions 10] [--out profiles/sgpmc_comp_rates.json]
"""
import argparse
import collections
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "experiments"))
import ggp_amd  # noqa: E402
from co2_composite_hmc import synthetic_keeling  # noqa: E402

N, D, M = 600, 1, 200


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median": round(statistics.median(ms), 4), "q1": round(q[0], 4), "q3": round(q[2], 4), "reps": len(ms)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def launches(fn, evals=5):
    """{name: launches per evaluation} of the device activity torch.profiler records, kernels and copies apart."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(evals):
            fn()
        torch.cuda.synchronize()
    kernels, copies = collections.Counter(), collections.Counter()
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            (copies if ev.name.startswith(("Memcpy", "Memset")) else kernels)[ev.name.split("(")[0]] += 1
    per = lambda c: {k: round(v / evals, 2) for k, v in sorted(c.items())}
    torch_side = lambda k: "at::" in k or "rocblas" in k          # torch's own launches (the mean function, the reductions into the result
    tch = {k: v for k, v in kernels.items() if torch_side(k)}     # buffer, its copies); everything else is the library's
    lib = {k: v for k, v in kernels.items() if not torch_side(k)}
    return {"kernels_per_evaluation": round(sum(kernels.values()) / evals, 2), "library_kernels_per_evaluation": round(sum(lib.values()) / evals, 2),
            "torch_kernels_per_evaluation": round(sum(tch.values()) / evals, 2), "copies_per_evaluation": round(sum(copies.values()) / evals, 2),
            "library_kernels": per(lib), "torch_kernels": per(tch), "copies": per(copies)}


def difference(a, b):
    """{kernel: launches per evaluation in a minus in b} where they differ: the launches that account for a time ratio above the count ratio."""
    ka, kb = dict(a["library_kernels"], **a["torch_kernels"]), dict(b["library_kernels"], **b["torch_kernels"])
    return {k: round(ka.get(k, 0.0) - kb.get(k, 0.0), 2) for k in sorted(set(ka) | set(kb)) if ka.get(k, 0.0) != kb.get(k, 0.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--transitions", type=int, default=10)
    ap.add_argument("--out", default="profiles/sgpmc_comp_rates.json")
    a = ap.parse_args()
    eng = ggp_amd.HipEngine()
    y_tr, t_tr, _, _, _ = synthetic_keeling()
    X = torch.as_tensor(t_tr[:N], dtype=torch.float64).to(eng.device)
    y = torch.as_tensor(y_tr[:N], dtype=torch.float64).to(eng.device)
    Z = X[torch.linspace(0, N - 1, M).round().long()].clone()
    new = ggp_amd.CompositeSgpmcTarget(X, y, Z, ggp_amd.co2_sgpmc_kernel(), priors=ggp_amd.CO2_SGPMC_PRIORS, white=1.0, mean="linear",
                                       engine=eng)
    bound = ggp_amd.CollapsedBound(X, y, kernel="composite", jitter=1e-4, engine=eng)
    old = ggp_amd.CompositeHmcTarget(bound, Z, ggp_amd.co2_kernel(), ggp_amd.CO2_LOG_PRIOR_SD)
    q_new = np.asarray(new.start())
    q_new[new.names.index("mean_A")] = 0.05      # a slope of the data's size: the start value 1 is 50 units off at t = 50
    q_old = list(old.start())
    fns = [lambda: new.logp_and_grad(q_new), lambda: old.logp_and_grad(q_old)]
    for fn in fns:
        lp, g = fn()
        assert math.isfinite(lp) and all(math.isfinite(t) for t in g), lp
    for _ in range(3):
        for fn in fns:
            fn()
    acc = [[], []]
    for _ in range(a.reps):
        for fn, t in zip(fns, acc):
            t.append(timed(fn))
    res = {"device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "shape": {"N": N, "d": D, "M": M},
           "ms_logp_and_grad_composite_sgpmc": spread(acc[0]), "ms_logp_and_grad_composite_collapsed_multi_launch": spread(acc[1]),
           "collapsed_single_launch": bool(bound._small_ok(M)),
           "ratio_sgpmc_over_collapsed": round(statistics.median(acc[0]) / statistics.median(acc[1]), 4)}
    try:
        ln, lo = launches(fns[0]), launches(fns[1])
        res.update(launches_composite_sgpmc=ln, launches_composite_collapsed=lo,
                   launch_count_ratio=round(ln["kernels_per_evaluation"] / lo["kernels_per_evaluation"], 4),
                   launches_sgpmc_minus_collapsed=difference(ln, lo))
    except Exception as e:  # noqa: BLE001 - a profiler that cannot start must not lose the timings
        res.update(launches_composite_sgpmc="not measured", launches_composite_collapsed="not measured", launch_count_ratio="not measured",
                   profiler_error=repr(e))
    t0 = time.perf_counter()
    tr = ggp_amd.sample_hmc(new, a.transitions, 0, seed=1, start=q_new, num_leapfrog_steps=20, step_size=0.005, num_adaptation_steps=20,
                            adaptation_rate=0.05)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    res.update(sample_hmc={"transitions": a.transitions, "num_leapfrog_steps": 20, "n_leapfrog": int(tr.n_leapfrog),
                           "transitions_per_s": round(a.transitions / secs, 3), "leapfrogs_per_s": round(tr.n_leapfrog / secs, 2),
                           "accept_rate": float(np.mean(tr.get_sampler_stats("is_accepted")))})
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
