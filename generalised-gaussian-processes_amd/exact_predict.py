"""The exact-GP mixture predictive over hyper-parameter draws on top of ``engine.exact_predict_batch`` + ``engine.exact_mixture``: what
the reference does with the draws of models/gpr_hmc.py (one predictive per draw, the RMSE of the mixture mean and the NLPD of the
mixture) for B data sets x S draws as ONE launch of each kernel (csrc/sgp_exact_predict.hip) and one host copy.

Marginal predictives only (mean and variance per test point); the full-covariance ``MultivariateNormal``s of
``full_mixture_posterior_predictive`` stay with ``GPR_HMC``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .exact_nuts import _host, _host_sets
from .ml2 import MAX_D, MAX_N, _check_kernel, _dev, _engine

NOISE_FLOOR_VAR, NOISE_FLOOR_SD = 1e-4, 0.01  # the reference's rule: a draw with sig_n^2 < 1e-4 is predicted at sig_n = 0.01


@dataclass
class ExactMixturePredictive:
    """``predict_exact_batch``'s result (numpy): the mixture over the kept draws of each of B data sets at its T test points."""
    mean: np.ndarray                   # B x T: the mixture mean
    var: np.ndarray                    # B x T: the mixture variance (within + between the draws)
    draw_mean: np.ndarray              # B x S x T
    draw_var: np.ndarray               # B x S x T
    info: np.ndarray                   # B x S: 0, or the pivot at which the draw's matrix failed (its rows are NaN; it is left out)
    kept: np.ndarray                   # B: draws in the mixture
    logpdf: Optional[np.ndarray]       # B x T: log of the mean over the draws of N(y_t | mu_st, v_st); None without Y_test
    mean_logpdf: Optional[np.ndarray]  # B x T: the mean over the draws of log N(y_t | mu_st, v_st); None without Y_test
    probs: Optional[np.ndarray] = None      # Q: the probabilities of a call with ``probs``
    quantiles: Optional[np.ndarray] = None  # B x Q x T: the mixture's quantiles at ``probs``
    pit: Optional[np.ndarray] = None        # B x T: the mixture CDF at y_t (a call with ``probs`` and Y_test)

    def _quantile_at(self, p):
        hit = [] if self.probs is None else np.flatnonzero(np.abs(self.probs - p) <= 1e-12)
        if len(hit) == 0:
            raise ValueError("the predictive has no quantile at p = %.6g: call predict with probs that hold it (got %s)"
                             % (p, None if self.probs is None else self.probs.tolist()))
        return self.quantiles[:, hit[0]]

    def interval(self, level=0.95):
        """(lower, upper), each B x T: the central interval of the mixture at ``level``, from the quantiles at (1 - level) / 2 and
        1 - (1 - level) / 2, both of which must be among ``probs``."""
        lo = 0.5 * (1.0 - level)
        return self._quantile_at(lo), self._quantile_at(1.0 - lo)

    def coverage(self, level=0.95):
        """B values: the share of test points with (1 - level) / 2 <= pit <= 1 - (1 - level) / 2 -- the target inside the central
        interval, from the mixture CDF alone (no quantile)."""
        if self.pit is None:
            raise ValueError("coverage needs the predictive of a call with probs and Y_test")
        lo = 0.5 * (1.0 - level)
        return ((self.pit >= lo) & (self.pit <= 1.0 - lo)).mean(1)

    def interval_width(self, level=0.95):
        """B values: the mean over the test points of the central interval's width."""
        lower, upper = self.interval(level)
        return (upper - lower).mean(1)

    def nlpd(self, Y_std=1.0):
        """B values: minus the mean over the test points of ``logpdf``, in the units of the unstandardised targets (+ log Y_std)."""
        if self.logpdf is None:
            raise ValueError("nlpd needs the predictive of a call with Y_test")
        return -self.logpdf.mean(1) + np.log(Y_std)

    def rmse(self, Y_test, Y_std=1.0):
        """B values: the root mean squared error of the mixture mean."""
        Y_test = np.asarray(Y_test, dtype=np.float64).reshape(self.mean.shape)
        return np.sqrt(((self.mean - Y_test) ** 2).mean(1)) * Y_std


def _mixture_frame(result, run, X, Y, Z, limits, theta, X_test, Y_test, kernel, engine, probs=None):
    """What the mixture predictives share: the host intake, the set index of every draw, the engine's batched predictive --
    ``run(eng, data, theta, Xt, idx)`` with ``data`` = (X, Y[, Z]) on the device and ``idx`` = (ix, iy[, iz], ixs), giving (mean, var,
    bound or None, info) --, ``exact_mixture`` over the draws of each data set, with ``probs`` one call of ``mixture_quantiles`` on
    the same device moments, and the ONE host copy into ``result``."""
    _check_kernel(kernel)
    eng = _engine(engine)
    Xh, Yh, Zh, B, N, d = _host_sets(X, Y, Z, limits)
    Xt = _host(X_test)
    Xt = Xt[:, None] if Xt.ndim == 1 else Xt
    theta = np.asarray(theta, dtype=np.float64)
    if Xt.shape[-1] != d or (Xt.ndim != 2 and Xt.shape[0] != B):
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
    held = [h for h in (Xh, Yh, Zh) if h is not None]
    idx = tuple(set_of if h is Yh or h.ndim != 2 else None for h in held + [Xt])  # a shared X, Z or X_test is set 0 for every draw
    mean, var, bound, info = run(eng, tuple(_dev(h, eng) for h in held), _dev(theta.reshape(B * S, d + 2), eng), _dev(Xt, eng), idx)
    Yt_d = None if Y_test is None else _dev(Yt, eng)
    mix = eng.exact_mixture(mean, var, info, [b * S for b in range(B + 1)], Ytest=Yt_d)
    # one host copy: everything in one float64 buffer (the integer columns are exact in it)
    parts = {"draw_mean": (mean, (B, S, T)), "draw_var": (var, (B, S, T)), "info": (info, (B, S))}
    if bound is not None:
        parts["bound"] = (bound, (B, S))
    parts.update(mean=(mix["mean"], (B, T)), var=(mix["var"], (B, T)), kept=(mix["kept"], (B,)))
    if Y_test is not None:
        parts.update(logpdf=(mix["logpdf"], (B, T)), mean_logpdf=(mix["mean_logpdf"], (B, T)))
    extra = {}
    if probs is not None:
        extra["probs"] = np.array(probs, dtype=np.float64).reshape(-1)
        mq = eng.mixture_quantiles(mean, var, info, [b * S for b in range(B + 1)], extra["probs"], Ytest=Yt_d)
        parts["quantiles"] = (mq["quantiles"], (B, extra["probs"].size, T))
        if Y_test is not None:
            parts["pit"] = (mq["pit"], (B, T))
    host = torch.cat([t.reshape(-1).to(torch.float64) for t, _ in parts.values()]).cpu().numpy()
    cuts = np.cumsum([0] + [int(np.prod(shape)) for _, shape in parts.values()])
    seg = {k: host[cuts[i]:cuts[i + 1]].reshape(shape) for i, (k, (_, shape)) in enumerate(parts.items())}
    seg.update(info=seg["info"].astype(np.int32), kept=seg["kept"].astype(np.int64))
    return result(**{"logpdf": None, "mean_logpdf": None, **seg, **extra})


def predict_theta_batch(X, Y, theta, X_test, Y_test=None, kernel="rbf", pred_noise=True, engine=None, probs=None) -> ExactMixturePredictive:
    """The mixture predictive at constrained rows: ``theta`` is B x S x (d + 2), rows [ls_1..d | sf2 | s2], used as they are.
    ``probs``: as in ``predict_exact_batch``."""
    def run(eng, data, th, Xt, idx):
        mean, var, info = eng.exact_predict_batch(*data, th, Xt, ix=idx[0], iy=idx[1], ixs=idx[2], kernel=kernel, pred_noise=pred_noise)
        return mean, var, None, info
    return _mixture_frame(ExactMixturePredictive, run, X, Y, None, (MAX_N, MAX_D, None), theta, X_test, Y_test, kernel, engine, probs)


def constrain_samples(samples, jitter=0.0):
    """theta rows [ls | sf2 | s2] of unconstrained positions [log ls | log sig_f | log sig_n] (..., d + 2), on a copy: s2 = sig_n^2 +
    jitter, with the reference's floor (sig_n^2 < 1e-4 -> sig_n = 0.01).  A NaN row stays NaN."""
    q = np.array(samples, dtype=np.float64)  # (a copy)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.exp(q)
        sn2 = v[..., -1] ** 2
        sn2 = np.where(sn2 < NOISE_FLOOR_VAR, NOISE_FLOOR_SD ** 2, sn2)
        return np.concatenate([v[..., :-2], v[..., -2:-1] ** 2, (sn2 + jitter)[..., None]], -1)


def predict_exact_batch(X, Y, samples, X_test, Y_test=None, kernel="rbf", jitter=0.0, pred_noise=True, engine=None,
                        probs=None) -> ExactMixturePredictive:
    """The mixture predictive of B exact GPs over S hyper-parameter draws each, on the device: one launch of the predictive kernel
    (B x S problems, one workgroup each), one of the mixture kernel, one host copy.

    X: N x d (shared) or B x N x d;  Y: B x N (or N);  X_test: T x d (shared) or B x T x d;  Y_test: B x T or None.  ``samples``: B x S
    x (d + 2) unconstrained positions [log ls | log sig_f | log sig_n] (``ExactNutsResult.samples`` flattened over the chains); theta =
    [exp, exp^2, exp^2 + jitter].  A draw with sig_n^2 < 1e-4 is predicted at sig_n = 0.01 (the reference's rule), on a copy: ``samples``
    is not modified.  A row with a NaN (a chain that had no start) fails the kernel's test of theta and is left out of the mixture
    (``info``, ``kept``), as is a draw whose matrix is not numerically positive definite.

    ``probs`` (1 to 8 probabilities in [1e-9, 1 - 1e-9]): one more launch on the device moments gives the mixture's ``quantiles`` at
    them (B x Q x T) and, with ``Y_test``, ``pit``, the mixture CDF at the targets -- ``interval``, ``coverage`` and
    ``interval_width`` of the result.  Without ``probs`` nothing more is launched."""
    samples = _host(samples)
    if samples.ndim == 2:
        samples = samples[None]
    return predict_theta_batch(X, Y, constrain_samples(samples, jitter), X_test, Y_test, kernel=kernel, pred_noise=pred_noise, engine=engine,
                               probs=probs)


def mixture_quantiles(draw_mean, draw_var, probs, info=None, y=None, engine=None):
    """Quantiles (and, with ``y``, the PIT) of the equal-weight mixture of the Gaussians N(draw_mean, draw_var) over the draws, for
    moments that are on the host: S x T (one data set) or B x S x T -- ``draw_mean`` / ``draw_var`` / ``info`` of an
    ``ExactMixturePredictive``, or the (f_means, y_stds ** 2) of ``predict_sgpmc``.  ``info`` (S or B x S, default all zero): a draw
    with info != 0 is left out.  ``y``: T or B x T targets.  One upload, one launch (``engine.mixture_quantiles``), one host copy.
    Returns (quantiles, pit or None): Q x T and T for S x T moments, B x Q x T and B x T otherwise."""
    eng = _engine(engine)
    mean, var = np.asarray(draw_mean, dtype=np.float64), np.asarray(draw_var, dtype=np.float64)
    if mean.ndim not in (2, 3) or var.shape != mean.shape or mean.shape[-2] < 1 or mean.shape[-1] < 1:
        raise ValueError("draw_mean and draw_var must both be S x T or B x S x T (got %s, %s)" % (mean.shape, var.shape))
    single = mean.ndim == 2
    B, S, T = (1,) + mean.shape if single else mean.shape
    info = np.zeros((B, S)) if info is None else np.asarray(info)
    if info.size != B * S:
        raise ValueError("info must be %d x %d (got %s)" % (B, S, info.shape))
    pr = np.array(probs, dtype=np.float64).reshape(-1)
    parts = [mean.reshape(-1), var.reshape(-1), (info.reshape(-1) != 0).astype(np.float64)]
    if y is not None:
        y = np.asarray(y, dtype=np.float64)
        if y.size != B * T or y.ndim != mean.ndim - 1:
            raise ValueError("y must be %s (got %s)" % ("T" if single else "B x T", y.shape))
        parts.append(y.reshape(-1))
    buf = _dev(np.concatenate(parts), eng)  # the one upload
    n = B * S * T
    res = eng.mixture_quantiles(buf[:n].view(B * S, T), buf[n:2 * n].view(B * S, T), buf[2 * n:2 * n + B * S].to(torch.int32),
                                [b * S for b in range(B + 1)], pr, Ytest=None if y is None else buf[2 * n + B * S:].view(B, T))
    out = [res["quantiles"].reshape(-1)] + ([res["pit"].reshape(-1)] if y is not None else [])
    host = torch.cat(out).cpu().numpy()  # the one copy
    quant = host[:B * pr.size * T].reshape(B, pr.size, T)
    pit = host[B * pr.size * T:].reshape(B, T) if y is not None else None
    return (quant[0], None if pit is None else pit[0]) if single else (quant, pit)
