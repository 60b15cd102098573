"""Generates tests/golden/sklearn/ml2_fits.npz and tests/golden/sklearn/lml_surface.npz: scikit-learn's multi-start ML-II fits and its
log-marginal-likelihood surfaces, the third-party pins of ``ggp_amd.fit_ml2`` and ``ggp_amd.lml_surface`` (tests/test_exact_batch.py on
the CPU double, tests/test_exact_batch_gpu.py on the device).

    GaussianProcessRegressor(kernel=ConstantKernel(1) * RBF(1 [ARD], (1e-2, 1e3)) + WhiteKernel(1 [, "fixed"]), alpha=0,
                             n_restarts_optimizer=10, random_state=seed).fit(X, y)

on 12 data sets per cell from ``ggp_amd.identification_data`` (sig_f = 5, lengthscale 2, sig_n = 1).  Stored per cell: X, Y, theta0,
bounds, the 10 restart points of every data set -- recorded from the optimiser calls of the fit itself and checked against
``check_random_state(seed).uniform(log lo, log hi)``, scikit-learn's rule -- its fitted kernel_.theta (converted to [ls | sf2 | s2]) and
log_marginal_likelihood_value_.  The script asserts, on the CPU double, the conditions tests/test_exact_batch.py states for every stored
data set; a seed whose data misses them is not written.

Run from the repository root:  python tests/golden/make_golden_ml2_sklearn.py
"""
import os
import sys

import numpy as np
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
from sklearn.utils import check_random_state

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ggp_amd  # noqa: E402
from exact_batch_double import ExactBatchDouble  # noqa: E402
from exact_batch_reference import reference  # noqa: E402

# (N, noise, d, seed)
CELLS = [(10, "fixed", 1, 0), (10, "learn", 1, 1), (40, "learn", 1, 2), (120, "fixed", 1, 3), (30, "learn", 2, 4)]
N_SETS, N_RESTARTS = 12, 10
LS_BOUNDS, AMP_BOUNDS = (1e-2, 1e3), (1e-5, 1e5)


class RecordingGPR(GaussianProcessRegressor):
    """Records the initial theta of every optimiser call of a fit."""

    def _constrained_optimization(self, obj_func, initial_theta, bounds):
        self.initial_thetas_.append(np.array(initial_theta))
        return super()._constrained_optimization(obj_func, initial_theta, bounds)


def to_ours(theta_log, d, noise):
    """scikit-learn's [log sf2 | log ls_1..d | log s2 (when free)] -> [ls_1..d | sf2 | s2]."""
    t = np.exp(theta_log)
    return np.concatenate([t[1:1 + d], t[:1], t[1 + d:] if noise == "learn" else [1.0]])


def projected_gradient_inf(X, y, theta, bounds, free, kernel="rbf"):
    """Infinity-norm of the projected gradient of -LML with respect to log theta, from the long-double reference."""
    d = X.shape[1]
    ref = reference(X, y, theta[:d], theta[d], theta[d + 1], kernel)
    z = np.log(theta)
    g = -(np.asarray(ref["g"], dtype=np.float64) * theta)
    pg = z - np.clip(z - g, np.log(bounds[:, 0]), np.log(bounds[:, 1]))
    return float(np.abs(pg[free]).max())


def check_fit(res, X, Y, bounds, noise, sk_lml):
    """The conditions of tests/test_exact_batch.py for one cell; returns a description of the first violation or None."""
    N = X.shape[0]
    free = np.ones(bounds.shape[0], dtype=bool)
    free[-1] = noise == "learn"
    for b in range(Y.shape[0]):
        if not res.lml[b] >= sk_lml[b] - 1e-6 * (abs(sk_lml[b]) + N):
            return "set %d: best lml %.12g below scikit-learn's %.12g" % (b, res.lml[b], sk_lml[b])
        if res.converged[b].sum() < 9:
            return "set %d: only %d of %d starts converged" % (b, res.converged[b].sum(), res.converged.shape[1])
        for s in np.nonzero(res.converged[b])[0]:
            pg = projected_gradient_inf(X, Y[b], res.theta_all[b, s], bounds, free)
            if not pg <= 1e-4:
                return "set %d start %d: projected gradient %.3g" % (b, s, pg)
    return None


def fit_cell(N, noise, d, seed):
    rng = np.random.default_rng(1000 + seed)
    X, Y, _ = ggp_amd.identification_data(N, N_SETS, rng, sig_sd=5.0, lengthscale=2.0, noise_sd=1.0, uniform=True, d=d)
    theta0 = np.array([1.0] * d + [1.0, 1.0])
    bounds = np.array([LS_BOUNDS] * d + [AMP_BOUNDS, AMP_BOUNDS])
    starts = np.zeros((N_SETS, N_RESTARTS, d + 2))
    sk_theta = np.zeros((N_SETS, d + 2))
    sk_lml = np.zeros(N_SETS)
    seeds = np.arange(N_SETS) + 100 * seed
    for b in range(N_SETS):
        k = ConstantKernel(1.0, AMP_BOUNDS) * RBF([1.0] * d if d > 1 else 1.0, LS_BOUNDS) \
            + WhiteKernel(1.0, "fixed" if noise == "fixed" else AMP_BOUNDS)
        gp = RecordingGPR(kernel=k, alpha=0.0, n_restarts_optimizer=N_RESTARTS, random_state=int(seeds[b]))
        gp.initial_thetas_ = []
        gp.fit(X, Y[b])
        lo, hi = gp.kernel_.bounds[:, 0], gp.kernel_.bounds[:, 1]
        r = check_random_state(int(seeds[b]))
        drawn = [r.uniform(lo, hi) for _ in range(N_RESTARTS)]
        assert len(gp.initial_thetas_) == 1 + N_RESTARTS and np.array_equal(np.array(drawn), np.array(gp.initial_thetas_[1:]))
        starts[b] = [to_ours(t, d, noise) for t in drawn]
        sk_theta[b] = to_ours(gp.kernel_.theta, d, noise)
        sk_lml[b] = gp.log_marginal_likelihood_value_
    res = ggp_amd.fit_ml2(X, Y, noise=noise, theta0=theta0, bounds=bounds, starts=starts, engine=ExactBatchDouble())
    return dict(X=X, Y=Y, theta0=theta0, bounds=bounds, starts=starts, sk_theta=sk_theta, sk_lml=sk_lml, seeds=seeds,
                noise=np.array(noise)), check_fit(res, X, Y, bounds, noise, sk_lml), res


def surfaces():
    out = {}
    rng = np.random.default_rng(7)
    latent = None
    grids = {"a": (5, np.logspace(-1, 3, 12), np.logspace(-1, 1, 12)), "b": (10, np.logspace(-1, 4, 12), np.logspace(-1, 4, 12))}
    for name, (N, sf2, ls) in grids.items():
        X, Y, latent = ggp_amd.identification_data(N, 1, rng, latent=latent)
        k = ConstantKernel(1.0, AMP_BOUNDS) * RBF(1.0, (1e-2, 1e4)) + WhiteKernel(1.0, "fixed")
        gp = GaussianProcessRegressor(kernel=k, alpha=0.0, optimizer=None).fit(X, Y[0])
        lml = np.array([[gp.log_marginal_likelihood(np.log([a, b])) for b in ls] for a in sf2])  # [sf2, ls]
        out.update({name + "_X": X, name + "_y": Y[0], name + "_sf2": sf2, name + "_ls": ls, name + "_s2": np.array(1.0),
                    name + "_lml": lml})
    return out


def main():
    out = {"n_cells": np.array(len(CELLS))}
    for c, (N, noise, d, seed) in enumerate(CELLS):
        for attempt in range(5):
            cell, problem, res = fit_cell(N, noise, d, seed + 10 * attempt)
            print("cell %d (N=%d %s d=%d) seed %d: %s; %d batched evaluations, best-of-starts minus scikit-learn's in [%.2e, %.2e]" % (
                c, N, noise, d, seed + 10 * attempt, problem or "ok", res.n_batches, (res.lml - cell["sk_lml"]).min(),
                (res.lml - cell["sk_lml"]).max()))
            if problem is None:
                break
            assert d > 1, "a 1-D cell misses the conditions: " + problem  # (only the 2-D cell may look for another seed)
        else:
            raise AssertionError("no seed of cell %d meets the conditions" % c)
        out.update({"c%d_%s" % (c, k): v for k, v in cell.items()})
    os.makedirs(os.path.join(HERE, "sklearn"), exist_ok=True)
    path = os.path.join(HERE, "sklearn", "ml2_fits.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    path = os.path.join(HERE, "sklearn", "lml_surface.npz")
    np.savez_compressed(path, **surfaces())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
