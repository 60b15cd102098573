"""Generates tests/golden/sklearn/exact_lml.npz: the exact GP log marginal likelihood and its gradient from scikit-learn, the
third-party pin of sgp_exact_eval (tests/test_gpr_hmc.py on the CPU double, tests/test_gpr_hmc_gpu.py on the device).

    GaussianProcessRegressor(kernel=ConstantKernel(sf2) * {RBF, Matern(nu=1.5), Matern(nu=2.5)}(ls, ARD) + WhiteKernel(s2),
                             alpha=0, optimizer=None).log_marginal_likelihood(theta, eval_gradient=True)

sklearn's theta is [log sf2, log ls_1..d, log s2] and its gradient is with respect to those logs; the file stores it as it comes
(the tests convert).  alpha=0: no regulariser beyond WhiteKernel, the density log N(y | 0, K + s2 I) of pm.gp.Marginal.

Run from the repository root:  python tests/golden/make_golden_exact_sklearn.py
"""
import os

import numpy as np
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel

HERE = os.path.dirname(os.path.abspath(__file__))
# (N, d, kernel, seed) -- theta drawn around the priors of the reference's model (ls ~ Gamma(2, 1), HalfCauchy scales)
CELLS = [(30, 1, "rbf", 0), (50, 3, "matern32", 1), (80, 6, "matern52", 2), (100, 8, "rbf", 3), (120, 13, "matern32", 4)]


def base_kernel(name, ls):
    if name == "rbf":
        return RBF(length_scale=ls)
    return Matern(length_scale=ls, nu=1.5 if name == "matern32" else 2.5)


def main():
    out = {"n_cells": np.array(len(CELLS))}
    for c, (N, d, kern, seed) in enumerate(CELLS):
        rng = np.random.default_rng(100 + seed)
        X = rng.standard_normal((N, d))
        y = np.sin(X.sum(1)) + 0.3 * rng.standard_normal(N)
        ls = rng.gamma(2.0, 1.0, d) + 0.3 * np.sqrt(d)
        sf2 = float(rng.uniform(0.5, 2.0))
        s2 = float(rng.uniform(0.02, 0.5))
        k = ConstantKernel(sf2, (1e-9, 1e9)) * base_kernel(kern, ls) + WhiteKernel(s2, (1e-12, 1e9))
        gp = GaussianProcessRegressor(kernel=k, alpha=0.0, optimizer=None, normalize_y=False).fit(X, y)
        theta = gp.kernel_.theta
        assert np.allclose(np.exp(theta), np.concatenate([[sf2], ls, [s2]]))
        F, g = gp.log_marginal_likelihood(theta, eval_gradient=True)
        p = "c%d_" % c
        out.update({p + "X": X, p + "y": y, p + "ls": ls, p + "sf2": np.array(sf2), p + "s2": np.array(s2),
                    p + "kernel": np.array(kern), p + "F": np.array(F), p + "grad_log": np.asarray(g)})
    path = os.path.join(HERE, "sklearn", "exact_lml.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
