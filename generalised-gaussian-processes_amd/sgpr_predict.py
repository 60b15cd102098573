"""The sparse-GP mixture predictive over hyper-parameter draws on top of ``engine.vfe_predict_batch`` + ``engine.exact_mixture``: what
the reference does with the draws of models/bayesian_sgpr_hmc.py (one predictive of the collapsed sparse GP per draw, the RMSE of the
mixture mean and the NLPD of the mixture) for B data sets x S draws as ONE launch of each kernel (csrc/sgp_vfe_predict.hip,
csrc/sgp_exact_predict.hip) and one host copy.

Marginal predictives only (mean and variance per test point).  ``BayesianSparseGPR_HMC.mixture_posterior_predictive`` and
``models.mixture_posterior_predictive`` keep their own route (``sgp_mixture_predict``: full covariances, one data set at a time).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._lib import VFE_BATCH_MAX_D as MAX_D, VFE_BATCH_MAX_M as MAX_M, VFE_BATCH_MAX_N as MAX_N
from .exact_predict import ExactMixturePredictive, _host, _mixture_frame


@dataclass
class SgprMixturePredictive(ExactMixturePredictive):
    """``predict_sgpr_batch``'s result (numpy): ``ExactMixturePredictive``'s fields (``info``: 0, k in 1..M where K_uu failed at pivot
    k, M + k where B did; such a draw's rows are NaN and it is left out) plus the collapsed bound at every draw."""
    bound: Optional[np.ndarray] = None  # B x S: F at every draw (NaN where info != 0)


def predict_sgpr_theta_batch(X, Y, Z, theta, X_test, Y_test=None, kernel="rbf", jitter=1e-6, pred_noise=True,
                             engine=None, probs=None) -> SgprMixturePredictive:
    """The mixture predictive at constrained rows: ``theta`` is B x S x (d + 2), rows [ls_1..d | sf2 | s2], used as they are.
    ``probs``: as in ``predict_exact_batch``."""
    def run(eng, data, th, Xt, idx):
        return eng.vfe_predict_batch(*data, th, Xt, ix=idx[0], iy=idx[1], iz=idx[2], ixs=idx[3], kernel=kernel, jitter=jitter,
                                     pred_noise=pred_noise, want_bound=True)
    return _mixture_frame(SgprMixturePredictive, run, X, Y, Z, (MAX_N, MAX_D, MAX_M), theta, X_test, Y_test, kernel, engine, probs)


def constrain_sgpr_samples(samples):
    """theta rows [ls | sf2 | s2] of unconstrained positions [log ls | log sig_f | log sig_n] (..., d + 2), on a copy: [exp, exp^2,
    exp^2].  No noise floor and no jitter on the noise: the reference's sparse route has neither (the floor belongs to the exact
    model's mixture; the jitter of the sparse model goes on K_uu).  A NaN row stays NaN."""
    q = np.array(samples, dtype=np.float64)  # (a copy)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.exp(q)
        return np.concatenate([v[..., :-2], v[..., -2:] ** 2], -1)


def predict_sgpr_batch(X, Y, Z, samples, X_test, Y_test=None, kernel="rbf", jitter=1e-6, pred_noise=True,
                       engine=None, probs=None) -> SgprMixturePredictive:
    """The mixture predictive of B collapsed sparse GPs over S hyper-parameter draws each, on the device: one launch of the predictive
    kernel (B x S problems, one workgroup each), one of the mixture kernel, one host copy.

    X: N x d (shared) or B x N x d;  Y: B x N (or N);  Z: M x d (shared) or B x M x d;  X_test: T x d (shared) or B x T x d;  Y_test:
    B x T or None.  ``samples``: B x S x (d + 2) unconstrained positions [log ls | log sig_f | log sig_n] (``SgprNutsResult.samples``
    flattened over the chains); theta = [exp, exp^2, exp^2], with no noise floor; ``jitter`` goes on K_uu, as in the sampler.  A row
    with a NaN (a chain that had no start) fails the kernel's test of theta and is left out of the mixture (``info``, ``kept``), as is
    a draw whose K_uu or B is not numerically positive definite.  ``probs``: the mixture's quantiles and PIT, as in
    ``predict_exact_batch`` (one more launch; none without)."""
    samples = _host(samples)
    if samples.ndim == 2:
        samples = samples[None]
    return predict_sgpr_theta_batch(X, Y, Z, constrain_sgpr_samples(samples), X_test, Y_test, kernel=kernel, jitter=jitter,
                                    pred_noise=pred_noise, engine=engine, probs=probs)
