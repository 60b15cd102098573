#!/usr/bin/env python3
"""The reference's joint-HMC CO2 experiment (experiments/co2_sgpmc.py) on the HIP core: GPflow's SGPMC with

    Periodic(SE, period 1 fixed) * Matern52 + RationalQuadratic + SquaredExponential + Matern52 + White,   Linear mean,   Gaussian noise

and the reference's priors (``ggp_amd.CO2_SGPMC_PRIORS``), sampled over every hyper-parameter and the whitened inducing values by
fixed-length HMC (20 leapfrog steps, step 0.005, 20 adaptation steps; no warm-up, Z frozen).  As the reference: the first 600 months
train (:49), M = 200 inducing inputs drawn from them with replacement (:190; K_uu then carries duplicates, which jitter + white
regularise), 100 burn-in transitions and 100 draws (:193), the predictive of the first 50 draws.  ``--mauna PATH`` reads the real
``mauna.txt`` (not shipped); without it the synthetic Keeling-like series of experiments/co2_composite_hmc.py stands in.
Prints one JSON object.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ggp_amd  # noqa: E402
from co2_composite_hmc import synthetic_keeling  # noqa: E402

SEP_IDX = 600   # co2_sgpmc.py:49


def load(mauna, seed):
    if mauna:
        year, co2 = ggp_amd.datasets.read_mauna_txt(mauna)
        std = float(np.std(co2))
        y, t, data = (co2 - co2[0]) / std, (year - year[0])[:, None], "mauna.txt"
    else:
        y_a, t_a, y_b, t_b, std = synthetic_keeling(seed=seed)
        y, t, data = np.concatenate([y_a, y_b]), np.concatenate([t_a, t_b]), "synthetic Keeling-like series"
    return y[:SEP_IDX], t[:SEP_IDX], y[SEP_IDX:], t[SEP_IDX:], std, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mauna", default=None, help="path to mauna.txt (year co2, -99.99 = missing)")
    ap.add_argument("--num_inducing", type=int, default=200)
    ap.add_argument("--tune", type=int, default=100)
    ap.add_argument("--num_samples", type=int, default=100)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()

    y_tr, t_tr, y_te, t_te, std, data = load(args.mauna, 47)
    rng = np.random.RandomState(args.seed)
    Z = np.array(t_tr)[rng.randint(0, len(t_tr), args.num_inducing)]
    eng = ggp_amd.HipEngine()
    model, trace, wall = ggp_amd.train_sgp_hmc_composite((t_tr, y_tr), Z, ggp_amd.co2_sgpmc_kernel(), args.tune, args.num_samples,
                                                         priors=ggp_amd.CO2_SGPMC_PRIORS, mean="linear", white=1.0, engine=eng,
                                                         seed=args.seed)
    pred_mean, f_means, y_stds = ggp_amd.predict_sgpmc(model, trace, t_te)
    lower, upper = ggp_amd.get_posterior_predictive_uncertainty_intervals(f_means, y_stds)
    Yt = torch.as_tensor(y_te)
    names = [n for n in dict.fromkeys(model.target.names) if n != "mean_A"]
    out = {"config": "CO2, SGPMC + HMC (JointHMC), composite covariance + White, linear mean", "data": data, "N_train": int(len(y_tr)),
           "N_test": int(len(y_te)), "num_inducing": args.num_inducing, "distinct_inducing": int(len(np.unique(Z))), "jitter": model.jitter,
           "tune": args.tune, "num_samples": len(trace), "num_leapfrog_steps": 20, "wall_clock_secs": wall,
           "n_leapfrog": int(trace.n_leapfrog), "leapfrogs_per_s": trace.n_leapfrog / wall, "evaluations": int(model.target.n_evals),
           "accept_rate": float(np.mean(trace.get_sampler_stats("is_accepted"))), "final_step_size": float(trace.final_step_size),
           "posterior_mean": dict({n: float(np.mean(trace[n])) for n in names}, mean_A=[float(v) for v in np.mean(trace["mean_A"], 0)]),
           "test_rmse_ppm": float(ggp_amd.rmse(torch.as_tensor(pred_mean), Yt, std)),
           "test_nlpd_mixture": ggp_amd.negative_log_predictive_mixture_density(Yt, f_means, y_stds, std),
           "interval_coverage_95": float(np.mean((y_te >= lower) & (y_te <= upper))),
           "interval_mean_width_ppm": float(np.mean(upper - lower) * std)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
