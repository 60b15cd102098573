"""Joint NUTS (all_in_HMC) rates: device-resident (sgp_small_nuts_joint, one persistent launch) against host-driven hmc.NUTS over
the same single-launch evaluations, same seed, at two shapes -- Boston-shaped synthetic data (N 404, d 13, M 100, standardised)
and C2's shape (N 634, d 1, M 128).  Also what workgroup 0 of the device run spent per leaf in the wide sampler against the
evaluation (device clock, counters of sgp_small_nuts_joint).

    python tools/allin_rates.py [--tune 30] [--draws 20] [--out profiles/allin_rates.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggp_amd  # noqa: E402
from ggp_amd.hmc import DiagMassAdapter, NUTS, SplitMix  # noqa: E402


def shape(name, N, d, M, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    w = rng.standard_normal(d) / math.sqrt(d)
    y = np.sin(2.0 * X @ w) + 0.3 * X[:, 0] + 0.1 * rng.standard_normal(N)
    X = (X - X.mean(0)) / X.std(0)
    y = (y - y.mean()) / y.std()
    return name, X, y, X[rng.choice(N, M, replace=False)].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tune", type=int, default=30)
    ap.add_argument("--draws", type=int, default=20)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default="profiles/allin_rates.json")
    a = ap.parse_args()
    eng = ggp_amd.HipEngine()
    rows = []
    for name, X, y, Z in (shape("boston_shaped", 404, 13, 100, 1), shape("c2_shape", 634, 1, 128, 2)):
        N, d = X.shape
        M = Z.shape[0]
        Xd = torch.as_tensor(X).to(eng.device)
        yd = torch.as_tensor(y).to(eng.device)
        tgt = ggp_amd.JointHmcTarget(ggp_amd.CollapsedBound(Xd, yd, jitter=1e-6, engine=eng), M)
        q0 = np.concatenate([np.array(tgt.start()[:d + 2]), Z.reshape(-1)]) + SplitMix(a.seed).uniform(-0.1, 0.1, tgt.ndim)
        eng.small_nuts_joint(Xd, yd, M, q0, 2, 2, a.seed, max_treedepth=a.depth)  # warm-up: code objects, workspace
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = eng.small_nuts_joint(Xd, yd, M, q0, a.tune, a.draws, a.seed, max_treedepth=a.depth)
        dev_wall = time.perf_counter() - t0
        assert r["info"] == 0 and r["draws"] == a.tune + a.draws
        nuts = NUTS(tgt.logp_and_grad, tgt.ndim, max_treedepth=a.depth, rng=SplitMix(a.seed))
        q = q0.copy()
        t0 = time.perf_counter()
        lp, g = nuts._eval(q)
        nuts.mass = DiagMassAdapter(tgt.ndim, initial_mean=q)
        for it in range(a.tune + a.draws):
            q, lp, g, _ = nuts.draw(q, lp, g, it < a.tune)
        host_wall = time.perf_counter() - t0
        ev = r["evaluations"]
        row = {"shape": name, "N": N, "d": d, "M": M, "ndim": tgt.ndim, "tune": a.tune, "draws": a.draws, "max_treedepth": a.depth,
               "device": {"leapfrogs": ev, "seconds": dev_wall, "leapfrogs_per_s": ev / dev_wall,
                          "sampler_us_per_leaf": 1e6 * r["sampler_seconds"] / ev, "evaluation_us_per_leaf": 1e6 * r["eval_seconds"] / ev,
                          "sampler_over_evaluation": r["sampler_seconds"] / r["eval_seconds"]},
               "host_driven": {"leapfrogs": nuts.n_leapfrog, "seconds": host_wall, "leapfrogs_per_s": nuts.n_leapfrog / host_wall}}
        row["device_over_host_rate"] = row["device"]["leapfrogs_per_s"] / row["host_driven"]["leapfrogs_per_s"]
        print(json.dumps(row))
        rows.append(row)
    out = {"tool": "tools/allin_rates.py", "device_name": torch.cuda.get_device_name(0),
           "note": "sampler / evaluation: s_memrealtime ticks of workgroup 0 between its evaluations and during them", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
