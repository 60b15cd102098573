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
import torch

from ._lib import VFE_BATCH_MAX_D as MAX_D, VFE_BATCH_MAX_M as MAX_M, VFE_BATCH_MAX_N as MAX_N
from .exact_predict import ExactMixturePredictive, _host
from .ml2 import _check_kernel, _dev, _engine


@dataclass
class SgprMixturePredictive(ExactMixturePredictive):
    """``predict_sgpr_batch``'s result (numpy): ``ExactMixturePredictive``'s fields (``info``: 0, k in 1..M where K_uu failed at pivot
    k, M + k where B did; such a draw's rows are NaN and it is left out) plus the collapsed bound at every draw."""
    bound: Optional[np.ndarray] = None  # B x S: F at every draw (NaN where info != 0)


def predict_sgpr_theta_batch(X, Y, Z, theta, X_test, Y_test=None, kernel="rbf", jitter=1e-6, pred_noise=True,
                             engine=None) -> SgprMixturePredictive:
    """The mixture predictive at constrained rows: ``theta`` is B x S x (d + 2), rows [ls_1..d | sf2 | s2], used as they are."""
    _check_kernel(kernel)
    eng = _engine(engine)
    Yh = _host(Y)
    Yh = Yh[None] if Yh.ndim == 1 else Yh
    Xh, Zh, Xt = _host(X), _host(Z), _host(X_test)
    Xh = Xh[:, None] if Xh.ndim == 1 else Xh
    Zh = Zh[:, None] if Zh.ndim == 1 else Zh
    Xt = Xt[:, None] if Xt.ndim == 1 else Xt
    theta = np.asarray(theta, dtype=np.float64)
    B, N = Yh.shape
    d, M = Xh.shape[-1], Zh.shape[-2]
    shared_x, shared_z, shared_t = Xh.ndim == 2, Zh.ndim == 2, Xt.ndim == 2
    if not 1 <= N <= MAX_N or not 1 <= d <= MAX_D or Xh.shape[-2] != N or (not shared_x and Xh.shape[0] != B):
        raise ValueError("X must be N x d or B x N x d with 1 <= N <= %d, 1 <= d <= %d, Y B x N (got X %s, Y %s)"
                         % (MAX_N, MAX_D, Xh.shape, Yh.shape))
    if not 1 <= M <= MAX_M or Zh.shape[-1] != d or (not shared_z and Zh.shape[0] != B):
        raise ValueError("Z must be M x %d or %d x M x %d with 1 <= M <= %d (got %s)" % (d, B, d, MAX_M, Zh.shape))
    if Xt.shape[-1] != d or (not shared_t and Xt.shape[0] != B):
        raise ValueError("X_test must be T x %d or %d x T x %d (got %s)" % (d, B, d, Xt.shape))
    if theta.ndim != 3 or theta.shape[0] != B or theta.shape[2] != d + 2 or theta.shape[1] < 1:
        raise ValueError("the draws must be %d x S x %d (got %s)" % (B, d + 2, theta.shape))
    S, T = theta.shape[1], Xt.shape[-2]
    if Y_test is not None:
        Yt = _host(Y_test)
        Yt = Yt[None] if Yt.ndim == 1 else Yt
        if Yt.shape != (B, T):
            raise ValueError("Y_test must be %d x %d (got %s)" % (B, T, Yt.shape))
    set_of = np.repeat(np.arange(B, dtype=np.int32), S)
    mean, var, bound, info = eng.vfe_predict_batch(
        _dev(Xh, eng), _dev(Yh, eng), _dev(Zh, eng), _dev(theta.reshape(B * S, d + 2), eng), _dev(Xt, eng),
        ix=None if shared_x else set_of, iy=set_of, iz=None if shared_z else set_of, ixs=None if shared_t else set_of, kernel=kernel,
        jitter=jitter, pred_noise=pred_noise, want_bound=True)
    mix = eng.exact_mixture(mean, var, info, [b * S for b in range(B + 1)], Ytest=None if Y_test is None else _dev(Yt, eng))
    # one host copy: everything in one float64 buffer (the integer columns are exact in it)
    parts = [mean.reshape(-1), var.reshape(-1), info.reshape(-1).to(torch.float64), bound.reshape(-1), mix["mean"].reshape(-1),
             mix["var"].reshape(-1), mix["kept"].reshape(-1).to(torch.float64)]
    if Y_test is not None:
        parts += [mix["logpdf"].reshape(-1), mix["mean_logpdf"].reshape(-1)]
    host = torch.cat(parts).cpu().numpy()
    cuts = np.cumsum([0, B * S * T, B * S * T, B * S, B * S, B * T, B * T, B] + ([B * T, B * T] if Y_test is not None else []))
    seg = [host[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)]
    return SgprMixturePredictive(
        mean=seg[4].reshape(B, T), var=seg[5].reshape(B, T), draw_mean=seg[0].reshape(B, S, T), draw_var=seg[1].reshape(B, S, T),
        info=seg[2].astype(np.int32).reshape(B, S), kept=seg[6].astype(np.int64),
        logpdf=seg[7].reshape(B, T) if Y_test is not None else None, mean_logpdf=seg[8].reshape(B, T) if Y_test is not None else None,
        bound=seg[3].reshape(B, S))


def constrain_sgpr_samples(samples):
    """theta rows [ls | sf2 | s2] of unconstrained positions [log ls | log sig_f | log sig_n] (..., d + 2), on a copy: [exp, exp^2,
    exp^2].  No noise floor and no jitter on the noise: the reference's sparse route has neither (the floor belongs to the exact
    model's mixture; the jitter of the sparse model goes on K_uu).  A NaN row stays NaN."""
    q = np.array(samples, dtype=np.float64)  # (a copy)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.exp(q)
        return np.concatenate([v[..., :-2], v[..., -2:] ** 2], -1)


def predict_sgpr_batch(X, Y, Z, samples, X_test, Y_test=None, kernel="rbf", jitter=1e-6, pred_noise=True,
                       engine=None) -> SgprMixturePredictive:
    """The mixture predictive of B collapsed sparse GPs over S hyper-parameter draws each, on the device: one launch of the predictive
    kernel (B x S problems, one workgroup each), one of the mixture kernel, one host copy.

    X: N x d (shared) or B x N x d;  Y: B x N (or N);  Z: M x d (shared) or B x M x d;  X_test: T x d (shared) or B x T x d;  Y_test:
    B x T or None.  ``samples``: B x S x (d + 2) unconstrained positions [log ls | log sig_f | log sig_n] (``SgprNutsResult.samples``
    flattened over the chains); theta = [exp, exp^2, exp^2], with no noise floor; ``jitter`` goes on K_uu, as in the sampler.  A row
    with a NaN (a chain that had no start) fails the kernel's test of theta and is left out of the mixture (``info``, ``kept``), as is
    a draw whose K_uu or B is not numerically positive definite."""
    samples = _host(samples)
    if samples.ndim == 2:
        samples = samples[None]
    return predict_sgpr_theta_batch(X, Y, Z, constrain_sgpr_samples(samples), X_test, Y_test, kernel=kernel, jitter=jitter,
                                    pred_noise=pred_noise, engine=engine)
