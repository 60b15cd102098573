#!/usr/bin/env python3
"""BASELINE config C1 -- the reference's 1-D demo (experiments/demo_1d_regression.py:55-139) on the HIP core.

Same data recipe (seeded torch RNG, train on |x| > 2, test grid linspace(-8, 8, 1000), Z_init = randn(25)),
same two models (SparseGPR with 2000 Adam steps at lr 0.01; BayesianSparseGPR_HMC with the
[100, 200, 500, 1000, 1500, 1999] HMC schedule), same metrics.  The GPflow "JointHMC" third panel (:145-164: SGPMC + HMC, 500 burn-in
transitions and 500 draws) is added to the JSON object by ``--joint_hmc`` (off by default: without the flag the output is unchanged; ``--joint_hmc_likelihood``
runs it on labels or counts drawn from the same latent function, through the Bernoulli or Poisson likelihood);
the plots are out of scope.  Prints one JSON object (keys follow experiments/regression.py:157-179).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggp_amd  # noqa: E402
from ggp_amd import BayesianSparseGPR_HMC, GaussianLikelihood, SparseGPR, mixture_posterior_predictive  # noqa: E402
from ggp_amd import nlpd, nlpd_mixture, rmse  # noqa: E402


def func(x):
    return torch.sin(x * 3) + 0.3 * torch.cos(x * 3.14)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max_iters", type=int, default=2000)
    ap.add_argument("--num_inducing", type=int, default=25)
    ap.add_argument("--skip_hmc", action="store_true")
    ap.add_argument("--joint_hmc", action="store_true", help="also the third panel: SGPMC + HMC (train_sgp_hmc / predict_sgpmc)")
    ap.add_argument("--joint_tune", type=int, default=500)
    ap.add_argument("--joint_samples", type=int, default=500)
    ap.add_argument("--joint_hmc_likelihood", choices=["gaussian", "bernoulli", "bernoulli_logit", "poisson"], default="gaussian",
                    help="likelihood of the third panel: labels (sign of the latent function + noise) or counts (Poisson(exp f)) are drawn "
                         "from the demo's latent function at the training inputs")
    args = ap.parse_args()

    torch.manual_seed(45)
    N = 1000
    X = torch.randn(N) * 2 - 1
    Y = func(X) + 0.4 * torch.randn(N)
    idx = (X < -2) | (X > 2)
    dev = torch.device("cuda", 0)
    X_train, Y_train = X[idx][:, None].double().to(dev), Y[idx].double().to(dev)
    X_test = torch.linspace(-8, 8, 1000).double()
    Y_test = func(X_test)
    Z_init = torch.randn(args.num_inducing).double()
    ystd = torch.tensor([1.0])
    out = {"N_train": int(idx.sum()), "num_inducing": args.num_inducing, "max_iters": args.max_iters}

    model = SparseGPR(X_train, Y_train, GaussianLikelihood(), Z_init, jitter=1e-6)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    t0 = time.time()
    losses = model.train_model(opt, max_steps=args.max_iters, verbose=False)
    wall = time.time() - t0
    pred = model.posterior_predictive(X_test.to(dev))
    # one record per model in the reference's result schema (experiments/regression.py:157-179)
    out["SparseGPR"] = ggp_amd.experiment_tools.result_record(
        "demo_1d", "SGPR", float(rmse(pred.loc, Y_test, ystd)), float(nlpd(pred, Y_test, ystd)), wall, num_inducing=args.num_inducing,
        max_iter=args.max_iters, final_loss=losses[-1],
        lengthscale=model.base_covar_module.base_kernel.lengthscale.detach().cpu().reshape(-1).tolist(),
        outputscale=float(model.base_covar_module.outputscale.detach()), noise=float(model.likelihood.noise.detach()))

    if not args.skip_hmc:
        hmc = BayesianSparseGPR_HMC(X_train, Y_train, GaussianLikelihood(), Z_init, jitter=1e-6, seed=45)
        opt = torch.optim.Adam(hmc.parameters(), lr=0.01)
        sched = [s for s in (100, 200, 500, 1000, 1500, 1999) if s < args.max_iters] or [args.max_iters - 1]
        t0 = time.time()
        losses, trace, step_sizes, perf = hmc.train_model(opt, max_steps=args.max_iters, hmc_scheduler=sched, verbose=False)
        wall = time.time() - t0
        preds = mixture_posterior_predictive(hmc, X_test.to(dev), trace)
        means = torch.stack([p.loc.cpu() for p in preds]).mean(0)
        out["BayesianSGPR_HMC"] = ggp_amd.experiment_tools.result_record(
            "demo_1d", "Bayesian_SGPR_HMC", float(rmse(means, Y_test, ystd)), float(nlpd_mixture(preds, Y_test, ystd)), wall,
            perf_times=perf, step_sizes=step_sizes, num_inducing=args.num_inducing, max_iter=args.max_iters, n_mixture=len(preds),
            ls_mean=float(np.mean(trace["ls"])), sig_n_mean=float(np.mean(trace["sig_n"])),
            leapfrogs_last_phase=int(trace.n_leapfrog), sampler_on_device=bool(getattr(trace, "device_resident", False)))
    if args.joint_hmc and args.joint_hmc_likelihood != "gaussian":
        # the non-conjugate case SGPMC exists for: labels / counts from the same latent function (the reference's data generator draws
        # them the same way, utils/load_data.py:61-62, 89-99), the likelihood's conditional moments of y per draw as the predictive
        lik = args.joint_hmc_likelihood
        gen = torch.Generator().manual_seed(45)
        f_train = func(X[idx]).double()
        if lik == "poisson":
            Y_lik = torch.poisson(torch.exp(f_train), generator=gen)
            truth = torch.exp(func(X_test)).numpy()
        else:
            link = (lambda f: 0.5 * torch.erfc(-f / 2 ** 0.5)) if lik == "bernoulli" else torch.sigmoid
            Y_lik = (torch.rand(f_train.shape, generator=gen, dtype=torch.float64) < link(f_train)).double()
            truth = link(func(X_test)).numpy()
        t0 = time.time()
        jm, jtrace, sample_secs = ggp_amd.train_sgp_hmc((X_train, Y_lik.to(dev)), Z_init[:, None], 1, args.joint_tune, args.joint_samples, seed=45,
                                                        likelihood=lik)
        wall = time.time() - t0
        pred_mean, y_means, y_stds = ggp_amd.predict_sgpmc(jm, jtrace, X_test[:, None])
        inside = np.abs(X_test.numpy()) > 2          # where there is training data
        out["JointHMC"] = ggp_amd.experiment_tools.result_record(
            "demo_1d", "JointHMC_" + lik, float(np.sqrt(np.mean((pred_mean - truth) ** 2))), float("nan"), wall, sampling_secs=sample_secs,
            rmse_where_trained=float(np.sqrt(np.mean((pred_mean - truth)[inside] ** 2))), likelihood=lik,
            num_inducing=args.num_inducing, tune=args.joint_tune, num_samples=args.joint_samples, n_mixture=int(y_means.shape[0]),
            acceptance=float(np.mean(jtrace.get_sampler_stats("is_accepted"))), step_size=float(jtrace.get_sampler_stats("step_size")[-1]),
            warmup=jm.warmup, lengthscale_mean=float(np.mean(jtrace["lengthscales"])), y_std_mean=float(np.mean(y_stds)))
    elif args.joint_hmc:
        # demo_1d_regression.py:160-164,213-217 of the reference; the mixture NLPD is the metric its SGPMC driver reports (models/sgp_hmc.py:154)
        t0 = time.time()
        jm, jtrace, sample_secs = ggp_amd.train_sgp_hmc((X_train, Y_train[:, None]), Z_init[:, None], 1, args.joint_tune, args.joint_samples, seed=45)
        wall = time.time() - t0
        pred_mean, f_means, y_stds = ggp_amd.predict_sgpmc(jm, jtrace, X_test[:, None])
        lower, upper = ggp_amd.get_posterior_predictive_uncertainty_intervals(f_means, y_stds)
        out["JointHMC"] = ggp_amd.experiment_tools.result_record(
            "demo_1d", "JointHMC", float(rmse(torch.as_tensor(pred_mean), Y_test, ystd)),
            float(ggp_amd.negative_log_predictive_mixture_density(Y_test, f_means, y_stds, 1.0)), wall, sampling_secs=sample_secs,
            num_inducing=args.num_inducing, tune=args.joint_tune, num_samples=args.joint_samples, n_mixture=int(f_means.shape[0]),
            acceptance=float(np.mean(jtrace.get_sampler_stats("is_accepted"))), step_size=float(jtrace.get_sampler_stats("step_size")[-1]),
            warmup=jm.warmup, lengthscale_mean=float(np.mean(jtrace["lengthscales"])), noise_variance_mean=float(np.mean(jtrace["noise_variance"])),
            coverage_95=float(np.mean((Y_test.numpy() >= lower) & (Y_test.numpy() <= upper))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
