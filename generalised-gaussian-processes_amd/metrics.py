"""Accuracy metrics with the reference's definitions (utils/metrics.py:38-67)."""
from __future__ import annotations

import math

import numpy as np
import torch


def _std(Y_std):
    return float(torch.as_tensor(Y_std).reshape(-1)[0])


def rmse(Y_pred_mean, Y_test, Y_std):
    """utils/metrics.py:38-40."""
    d = Y_pred_mean.detach().to("cpu", torch.float64) - Y_test.detach().to("cpu", torch.float64)
    return _std(Y_std) * torch.sqrt(torch.mean(d ** 2))


def nlpd(Y_test_pred, Y_test, Y_std):
    """Joint predictive log-density / n_test, rescaled (utils/metrics.py:42-47; note: joint, not marginal)."""
    lpd = Y_test_pred.log_prob(Y_test)
    return -(lpd.detach() / len(Y_test) - math.log(_std(Y_std)))


def nlpd_marginal(Y_test_pred, Y_test, Y_std):
    """Mean of the per-point Gaussian log-densities (utils/metrics.py:49-58)."""
    y = Y_test.detach().to("cpu", torch.float64).numpy()
    mu = Y_test_pred.loc.detach().to("cpu", torch.float64).numpy()
    var = Y_test_pred.variance.detach().to("cpu", torch.float64).numpy()
    lp = -0.5 * np.log(2.0 * np.pi * var) - 0.5 * (y - mu) ** 2 / var - math.log(_std(Y_std))
    return float(-np.mean(lp))


def nlpd_mixture(Y_test_pred_list, Y_test, Y_std):
    """Mean over the per-sample joint nlpd (utils/metrics.py:61-67)."""
    return float(np.mean([float(nlpd(p, Y_test, Y_std)) for p in Y_test_pred_list]))


def negative_log_predictive_mixture_density(Y_test, y_mix_loc, y_mix_std, Y_std):
    """The metric the reference's SGPMC driver reports (utils/metrics.py:70-78, called at models/sgp_hmc.py:154).  ``y_mix_loc`` /
    ``y_mix_std`` are (components x test points).  As in the reference it is the MEAN OVER COMPONENTS OF THE LOG-densities per test
    point (not the log of the mean density), minus log ``Y_std``, averaged over the test points, rounded to three decimals and negated."""
    y = np.asarray(torch.as_tensor(Y_test).detach().to("cpu", torch.float64)).reshape(-1)
    loc = np.asarray(y_mix_loc, dtype=np.float64)
    std = np.asarray(y_mix_std, dtype=np.float64)
    if loc.shape != std.shape or loc.ndim != 2 or loc.shape[1] != y.shape[0]:
        raise ValueError("y_mix_loc / y_mix_std must both be (components, %d), got %s and %s" % (y.shape[0], loc.shape, std.shape))
    lp = -0.5 * np.log(2.0 * np.pi * std ** 2) - 0.5 * ((y[None, :] - loc) / std) ** 2 - math.log(_std(Y_std))
    return float(-np.round(np.mean(np.mean(lp, axis=0)), 3))
