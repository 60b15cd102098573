#!/usr/bin/env python3
"""The 1-D multi-class demo: the data generator's ``multi-class`` recipe (utils/load_data.py:67-113 with ``classes=3``) through SGPMC +
HMC with the robust-max likelihood.

The recipe, restated with torch / numpy and seeded: 200 inputs on [0, 10], an RBF kernel with lengthscale 0.5, one latent function per
class drawn from N(0, K + 1e-6 I), y = argmax over the classes, 40 training inputs chosen uniformly without replacement; the other
160 are held out.  ``train_sgp_hmc(likelihood="multiclass")`` warms up (L-BFGS over everything, Z included), samples, and
``predict_sgpmc`` returns the class probabilities per draw.  Prints one JSON record with the held-out accuracy and the mean log
predictive probability of the true class, beside the two baselines it has to clear: log(1 / C) and the majority-class frequency.

``--svgp`` adds the variational, minibatch model on the same data: ``StochasticVariationalGP`` with a ``RobustMaxLikelihood`` (one q(u_c)
per class, the bound and its gradients in sgp_svgp_mc_elbo), minibatch Adam over Z, the q(u_c) and the hyper-parameters; its held-out
accuracy and mean log predictive probability are printed next to the SGPMC figures.
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


def make_data(seed=3, n=200, n_train=40, classes=3, lengthscale=0.5):
    """(X_train, y_train, X_test, y_test) of the recipe above (float64 numpy; labels as floats 0 .. classes-1)."""
    gen = torch.Generator().manual_seed(int(seed))
    X = torch.linspace(0.0, 10.0, n, dtype=torch.float64)
    K = torch.exp(-0.5 * ((X[:, None] - X[None, :]) / lengthscale) ** 2) + 1e-6 * torch.eye(n, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    latent = L @ torch.randn(n, classes, dtype=torch.float64, generator=gen)
    y = torch.argmax(latent, 1).to(torch.float64)
    perm = torch.randperm(n, generator=gen)
    tr, te = perm[:n_train].sort().values, perm[n_train:].sort().values
    return X[tr].numpy(), y[tr].numpy(), X[te].numpy(), y[te].numpy()


def run(engine=None, seed=3, num_inducing=10, tune=100, num_samples=100, warmup_iters=50, classes=3, n_draws=50):
    """The record of one run on ``engine`` (None: the HIP engine on the current device)."""
    Xtr, ytr, Xte, yte = make_data(seed, classes=classes)
    Z0 = np.linspace(0.5, 9.5, num_inducing)[:, None]
    t0 = time.time()
    model, trace, sample_secs = ggp_amd.train_sgp_hmc((torch.as_tensor(Xtr)[:, None], torch.as_tensor(ytr)), torch.as_tensor(Z0), 1, tune,
                                                      num_samples, engine=engine, seed=seed, warmup_iters=warmup_iters,
                                                      likelihood="multiclass", num_classes=classes)
    wall = time.time() - t0
    pred_mean, probs, _ = ggp_amd.predict_sgpmc(model, trace, torch.as_tensor(Xte)[:, None], n_draws=n_draws)
    yi = yte.astype(np.int64)
    majority = int(np.bincount(ytr.astype(np.int64), minlength=classes).argmax())
    return {"experiment": "demo_1d_classification", "model": "JointHMC_multiclass", "classes": classes, "N_train": int(len(ytr)),
            "N_test": int(len(yte)), "num_inducing": int(num_inducing), "tune": int(tune), "num_samples": int(num_samples),
            "accuracy": float(np.mean(pred_mean.argmax(1) == yi)),
            "mean_log_pred_prob": float(np.mean(np.log(pred_mean[np.arange(len(yi)), yi]))),
            "baseline_log_uniform": float(np.log(1.0 / classes)), "baseline_majority_accuracy": float(np.mean(yi == majority)),
            "n_mixture": int(probs.shape[0]), "acceptance": float(np.mean(trace.get_sampler_stats("is_accepted"))),
            "warmup": model.warmup, "wall_clock_secs": wall, "sampling_secs": sample_secs}


def run_svgp(engine=None, seed=3, num_inducing=10, steps=300, batch=20, lr=0.02, classes=3, n_train=40):
    """The record of one minibatch-Adam run of the multi-class SVGP model on ``engine`` (None: the HIP engine on the current device).
    (Step size 0.02: the factors LS_c are unconstrained, as in the single-class model, and at 0.05 Adam carries a diagonal entry through
    zero within 40 steps, where the KL term's logarithm is NaN.)"""
    Xtr, ytr, Xte, yte = make_data(seed, n_train=n_train, classes=classes)
    if engine is None:
        engine = ggp_amd.HipEngine(torch.device("cuda", 0))
    to = lambda a: torch.as_tensor(a).to(engine.device)  # noqa: E731
    X, y = to(Xtr)[:, None], to(ytr)
    Z0 = torch.as_tensor(np.linspace(0.5, 9.5, num_inducing)[:, None])
    model = ggp_amd.StochasticVariationalGP(X, y, ggp_amd.RobustMaxLikelihood(classes), Z0, num_tasks=classes, engine=engine)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X.cpu(), y.cpu()), batch_size=batch, shuffle=True,
                                         generator=torch.Generator().manual_seed(int(seed)))
    per_epoch = (len(ytr) + batch - 1) // batch
    t0 = time.time()
    losses = model.train_model(opt, loader, minibatch_size=batch, num_epochs=max(1, steps // per_epoch))
    wall = time.time() - t0
    probs = model.posterior_predictive(to(Xte)[:, None]).cpu().numpy()
    yi = yte.astype(np.int64)
    majority = int(np.bincount(ytr.astype(np.int64), minlength=classes).argmax())
    return {"experiment": "demo_1d_classification", "model": "SVGP_multiclass", "classes": classes, "N_train": int(len(ytr)),
            "N_test": int(len(yte)), "num_inducing": int(num_inducing), "steps": len(losses), "minibatch": int(batch),
            "accuracy": float(np.mean(probs.argmax(1) == yi)),
            "mean_log_pred_prob": float(np.mean(np.log(probs[np.arange(len(yi)), yi]))),
            "baseline_log_uniform": float(np.log(1.0 / classes)), "baseline_majority_accuracy": float(np.mean(yi == majority)),
            "first_loss": losses[0], "last_loss": losses[-1], "wall_clock_secs": wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--num_inducing", type=int, default=10)
    ap.add_argument("--tune", type=int, default=100)
    ap.add_argument("--num_samples", type=int, default=100)
    ap.add_argument("--warmup_iters", type=int, default=50)
    ap.add_argument("--svgp", action="store_true", help="also train the multi-class SVGP model (minibatch Adam) on the same data")
    ap.add_argument("--svgp_steps", type=int, default=300)
    ap.add_argument("--svgp_batch", type=int, default=20)
    args = ap.parse_args()
    rec = run(None, args.seed, args.num_inducing, args.tune, args.num_samples, args.warmup_iters)
    print(json.dumps(rec))
    if args.svgp:
        sv = run_svgp(None, args.seed, args.num_inducing, args.svgp_steps, args.svgp_batch)
        sv.update(sgpmc_accuracy=rec["accuracy"], sgpmc_mean_log_pred_prob=rec["mean_log_pred_prob"])
        print(json.dumps(sv))


if __name__ == "__main__":
    main()
