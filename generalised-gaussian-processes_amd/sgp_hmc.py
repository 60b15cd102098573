"""SGPMC + HMC ("JointHMC"): the third sampler row of the reference's tables (models/sgp_hmc.py; Hensman et al. 2015).

GPflow's ``SGPMC`` with a Gaussian likelihood (the reference's), or with a Bernoulli (probit / logit) or Poisson likelihood -- the
non-conjugate case SGPMC exists for -- sampled jointly over the hyper-parameters and the whitened inducing values by
fixed-length HMC with TFP's simple step-size adaptation.  Here the density is ``targets.SgpmcTarget`` (the whitened sufficient
statistics streamed by pass 1, the SGPMC tail of include/sgp.h, the factored pass 2) and the sampler ``hmc.sample_hmc``.

The reference's ``train_sgp_hmc`` returns ``(model, hmc_helper, samples, wall_clock_secs)`` and its callers unpack that tuple
inconsistently; ``hmc_helper`` (GPflow's ``SamplingHelper``) has no counterpart here.  The signatures chosen:
``train_sgp_hmc(...) -> (model, trace, wall_clock_secs)`` and ``predict_sgpmc(model, trace, X_test) -> (pred_mean, f_means, y_stds)``.
"""
from __future__ import annotations

import math
import time

import numpy as np
import torch

from .composite import CompositeSgpmcTarget
from .hmc import sample_hmc
from .targets import SgpmcTarget


class SgpmcModel:
    """What ``train_sgp_hmc`` and ``train_sgp_hmc_composite`` return as ``model``: the target (an ``SgpmcTarget`` or a
    ``CompositeSgpmcTarget``: data, kernel, jitter, engine), the inducing inputs (``Z``, frozen during sampling; the warm-up of
    ``train_sgp_hmc`` leaves them) and the warm-up's record."""

    def __init__(self, target):
        self.target = target
        self.engine = target.engine
        self.kernel = target.kernel
        self.jitter = target.jitter
        self.likelihood = target.likelihood
        self.warmup = {}

    @property
    def Z(self):
        return self.target.Z


CompositeSgpmcModel = SgpmcModel   # the name ``train_sgp_hmc_composite``'s model had while the two were separate classes


def _as_tensor(a):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(torch.float64)


def train_sgp_hmc(data, Z_init, input_dims, tune, num_samples, engine=None, seed=None, warmup_iters=100, likelihood="gaussian",
                  num_classes=None):
    """models/sgp_hmc.py:32-91.  ``data`` = (X_train, Y_train); returns ``(model, trace, wall_clock_secs)``.  ``likelihood``:
    "gaussian" (the reference's), "bernoulli" (probit), "bernoulli_logit", "poisson" or "multiclass" (robust-max over ``num_classes``
    latent GPs, labels 0 .. C-1; C = max label + 1 when not given) (``targets.SgpmcTarget``).

    As the reference: (1) a warm-up, ``scipy.optimize.minimize(method="L-BFGS-B", jac=True, maxiter=warmup_iters)`` on -logp over
    every variable INCLUDING the inducing inputs (:54-55; gpflow.optimizers.Scipy's default method); (2) Z is frozen (:56); (3)
    ``sample_hmc`` with ``tune`` burn-in transitions and ``num_samples`` draws from where the warm-up ended (:67-83: 10 leapfrog
    steps, step 0.01, 10 adaptation steps, target 0.8, rate 0.1).  ``wall_clock_secs`` times the sampling only (:86-88)."""
    from scipy.optimize import minimize
    X, Y = _as_tensor(data[0]), _as_tensor(data[1]).reshape(-1)
    if X.dim() == 1:
        X = X[:, None]
    Z0 = _as_tensor(Z_init)
    if Z0.dim() == 1:
        Z0 = Z0[:, None]
    if X.shape[1] != int(input_dims) or Z0.shape[1] != int(input_dims):
        raise ValueError("input_dims = %d, X has %d columns, Z_init has %d" % (int(input_dims), X.shape[1], Z0.shape[1]))
    target = SgpmcTarget(X, Y, Z0, kernel="rbf", jitter=1e-5, engine=engine, likelihood=likelihood,   # SquaredExponential, jitter 1e-5 (:20, :36)
                         **({"num_classes": num_classes} if likelihood == "multiclass" else {}))
    model = SgpmcModel(target)
    M, d, nd = target.M, target.d, target.ndim
    dev = target.engine.device

    def loss(w):
        target.set_Z(torch.from_numpy(w[nd:].reshape(M, d).copy()).to(dev))
        lp, g, gz = target.logp_and_grad(w[:nd], want_gz=True)
        if not math.isfinite(lp):
            return 1e100, np.zeros_like(w)
        return -lp, -np.concatenate([np.asarray(g, dtype=np.float64), gz.detach().to("cpu").numpy().reshape(-1)])

    w0 = np.concatenate([np.asarray(target.start(), dtype=np.float64), Z0.detach().to("cpu").numpy().reshape(-1)])
    f0 = loss(w0)[0]
    if int(warmup_iters) > 0:
        r = minimize(loss, w0, jac=True, method="L-BFGS-B", options={"maxiter": int(warmup_iters)})
        w1, f1, nit = (r.x, float(r.fun), int(r.nit)) if r.fun <= f0 else (w0, f0, 0)
    else:
        w1, f1, nit = w0, f0, 0
    target.set_Z(torch.from_numpy(w1[nd:].reshape(M, d).copy()).to(dev))   # frozen from here on
    model.warmup = {"loss_start": float(f0), "loss_end": float(f1), "iterations": nit}
    t0 = time.time()
    trace = sample_hmc(target, int(num_samples), int(tune), seed=seed, start=w1[:nd])
    wall_clock_secs = time.time() - t0
    return model, trace, wall_clock_secs


def train_sgp_hmc_composite(data, Z_init, kernel, tune, num_samples, priors=None, mean="linear", white=1.0, likelihood="gaussian",
                            engine=None, seed=None, num_leapfrog_steps=20, step_size=0.005, num_adaptation_steps=20, target_accept=0.8,
                            adaptation_rate=0.05):
    """experiments/co2_sgpmc.py:57-144: SGPMC with a sum-of-products ``kernel`` (``composite.CompositeKernel``), a White term
    (``white``: its start value, None for none), a linear mean function and per-parameter ``priors``
    (``composite.CompositeSgpmcTarget``); returns ``(model, trace, wall_clock_secs)``.  As the reference: jitter 1e-4 (:22), no warm-up
    (commented out, :105-107), Z frozen (:108), ``sample_hmc`` from the start values with 20 leapfrog steps, step 0.005, 20 adaptation
    steps, target 0.8, rate 0.05 (:120-126).  ``wall_clock_secs`` times the sampling only."""
    X, Y = _as_tensor(data[0]), _as_tensor(data[1]).reshape(-1)
    if X.dim() == 1:
        X = X[:, None]
    target = CompositeSgpmcTarget(X, Y, _as_tensor(Z_init), kernel, priors=priors, white=white, mean=mean, likelihood=likelihood,
                                  jitter=1e-4, engine=engine)
    model = CompositeSgpmcModel(target)
    t0 = time.time()
    trace = sample_hmc(target, int(num_samples), int(tune), seed=seed, start=target.start(), num_leapfrog_steps=num_leapfrog_steps,
                       step_size=step_size, num_adaptation_steps=num_adaptation_steps, target_accept=target_accept,
                       adaptation_rate=adaptation_rate)
    wall_clock_secs = time.time() - t0
    return model, trace, wall_clock_secs


def _log_ndtr(z):
    """log Phi(z), float64, finite down to where z^2 / 2 overflows (torch's routine: the host needs no erfcx of its own)."""
    return torch.special.log_ndtr(torch.as_tensor(np.asarray(z, dtype=np.float64))).numpy()


def likelihood_moments(likelihood, mu, var, eps=1e-3):
    """(E y, sd y) of y | f ~ likelihood with f ~ N(mu, var), elementwise:
    Bernoulli (y in {0, 1}): p and sqrt(p (1 - p)) with p = Phi(mu / sqrt(1 + var)) for the probit link, the 20-point Gauss-Hermite
    mean of sigmoid(f) for the logit link; Poisson (log link): m = exp(mu + var / 2) and sqrt(m + (e^var - 1) m^2).
    "multiclass" (robust-max): ``mu`` is (.., C), the latent means of the C classes, ``var`` (..) their shared variance; returns the
    class probabilities p_c = (1 - eps) P(c largest) + eps / (C - 1) (1 - P(c largest)), (.., C), with P(c largest) = sum_i w_i
    prod_{k != c} Phi(x_i + (mu_c - mu_k) / sqrt var) on the 20-point rule of the device code, and sqrt(p (1 - p))."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    if likelihood == "multiclass":
        Cn = mu.shape[-1]
        x, w = np.polynomial.hermite_e.hermegauss(20)
        w = w / math.sqrt(2.0 * math.pi)
        sd = np.sqrt(var)[..., None]
        lp = _log_ndtr(x[:, None, None] + ((mu[..., :, None] - mu[..., None, :]) / sd[..., None])[..., None, :, :])   # (.., 20, c, k)
        lp = lp * (1.0 - np.eye(Cn))                                                                                   # k != c
        P = np.einsum("i,...ic->...c", w, np.exp(lp.sum(-1)))
        p = (1.0 - eps) * P + eps / (Cn - 1) * (1.0 - P)
        return p, np.sqrt(p * (1.0 - p))
    if likelihood == "poisson":
        m = np.exp(mu + 0.5 * var)
        return m, np.sqrt(m + np.expm1(var) * m * m)
    if likelihood == "bernoulli":
        erf = np.vectorize(math.erf, otypes=[np.float64])
        p = 0.5 * (1.0 + erf(mu / np.sqrt(1.0 + var) / math.sqrt(2.0)))
    elif likelihood == "bernoulli_logit":
        x, w = np.polynomial.hermite_e.hermegauss(20)
        f = mu[..., None] + np.sqrt(var)[..., None] * x
        p = (0.5 * (1.0 + np.tanh(0.5 * f))) @ (w / math.sqrt(2.0 * math.pi))
    else:
        raise ValueError("no conditional moments for the likelihood %r" % (likelihood,))
    return p, np.sqrt(p * (1.0 - p))


def predict_sgpmc(model, trace, X_test, n_draws=50):
    """models/sgp_hmc.py:93-130: ``(pred_mean, f_means, y_stds)``, the last two (draws x test points).  The reference predicts from
    the FIRST 50 draws of the chain; ``n_draws`` keeps that default (fewer when the trace is shorter).  Per draw ``predict_f`` is the
    whitened SVGP predictive with q(v) a point mass, ``engine.svgp_predict(m=v, LS=0)``: mean = a^T v, var = k** - |a|^2 with
    a = L^-1 k_u*; y_std = sqrt(var + noise variance).  With a non-Gaussian likelihood ``f_means`` and ``y_stds`` hold the likelihood's
    conditional moments of y per draw (``likelihood_moments``) and ``pred_mean`` their mean over the draws.

    A model over a ``CompositeSgpmcTarget`` (``train_sgp_hmc_composite``) is predicted by ``sgpmc_comp_rows`` on X_test without labels, per draw:
    mean = a^T v + m(x*), var = kdiag + white - |a|^2."""
    e = model.engine
    Xs = _as_tensor(X_test)
    if Xs.dim() == 1:
        Xs = Xs[:, None]
    Xs = Xs.to(e.device).contiguous()
    n = min(int(n_draws), len(trace))
    if n <= 0:
        raise ValueError("the trace holds no draws")
    if isinstance(model.target, CompositeSgpmcTarget):
        per_draw = _predict_composite(model, trace, Xs, n)
    elif model.likelihood == "multiclass":
        per_draw = _predict_multiclass(model, trace, Xs, n)
    else:
        per_draw = _predict_stationary(model, trace, Xs, n)
    means, stds = (np.stack(a) for a in zip(*per_draw))
    return means.mean(0), means, stds


def _draw_moments(model, mean, var, s2):
    """(f_mean, y_std) of one draw from the latent mean and variance: y's own moments under a non-Gaussian likelihood."""
    if model.likelihood == "gaussian":
        return mean, np.sqrt(var + s2)
    return likelihood_moments(model.likelihood, mean, var)


def _predict_stationary(model, trace, Xs, n):
    e, Z = model.engine, model.Z
    M = int(Z.shape[0])
    LS = torch.zeros(M, M, dtype=torch.float64, device=e.device)
    out = []
    for i in range(n):
        row = trace[i]
        m = torch.as_tensor(np.asarray(row["V"], dtype=np.float64)).to(e.device).contiguous()
        mean, var, _ = e.svgp_predict(Xs, Z, [float(t) for t in np.asarray(row["lengthscales"]).reshape(-1)], float(row["variance"]), m, LS,
                                      jitter=model.jitter, kernel=model.kernel)
        mean, var = mean.detach().to("cpu").numpy(), np.maximum(var.detach().to("cpu").numpy(), 0.0)
        out.append(_draw_moments(model, mean, var, float(row["noise_variance"]) if model.likelihood == "gaussian" else None))
    return out


def _predict_multiclass(model, trace, Xs, n):
    """Per draw one ``sgpmc_mc_rows`` call without labels on the test rows (the C latent means and their shared variance), then the class
    probabilities on the host: per draw (probs (T x C), sqrt(p (1 - p)))."""
    e, t = model.engine, model.target
    Z = model.Z
    T, M = int(Xs.shape[0]), int(Z.shape[0])
    t_buf = e.kfu_buffer(T, M)
    out = []
    for i in range(n):
        row = trace[i]
        ls, sf2 = [float(v) for v in np.asarray(row["lengthscales"]).reshape(-1)], float(row["variance"])
        V = torch.as_tensor(np.asarray(row["V"], dtype=np.float64).reshape(t.num_classes, M)).to(e.device).contiguous()
        linv, _ = e.kuu_factor(e.kuu(Z, ls, sf2, model.jitter, model.kernel))
        r = e.sgpmc_mc_rows(Xs, None, Z, ls, sf2, V, linv, t_buf, model.kernel, t.eps)
        mu, var = r["mu"].detach().to("cpu").numpy().T, np.maximum(r["var"].detach().to("cpu").numpy(), sf2 * 2.0 ** -40)
        out.append(likelihood_moments("multiclass", mu, var, t.eps))
    return out


def _predict_composite(model, trace, Xs, n):
    e, t = model.engine, model.target
    Z, M, T = model.Z, int(model.Z.shape[0]), int(Xs.shape[0])
    t_buf = e.kfu_buffer(T, M)
    out = []
    for i in range(n):
        q = trace[i]["theta_unc"]
        block, white, s2, A, b, _ = t.unpack(q)
        linv, info = e.kuu_factor(e.kuu(Z, block, 1.0, model.jitter + white, "composite"))
        v = torch.as_tensor(np.asarray(q[t.n_theta:], dtype=np.float64)).to(e.device).contiguous()
        m = None if A is None else (Xs @ torch.tensor(A, dtype=torch.float64).to(e.device) + b).contiguous()
        r = e.sgpmc_comp_rows(Xs, None, Z, block, white, 1.0, v, linv, t_buf, model.likelihood, mean=m)
        mean, var = r["mu"].detach().to("cpu").numpy(), np.maximum(r["var"].detach().to("cpu").numpy(), 0.0)
        if int(info.item()) != 0:
            raise RuntimeError("K_uu of draw %d is not positive definite (status %d)" % (i, int(info.item())))
        out.append(_draw_moments(model, mean, var, s2))
    return out


def get_posterior_predictive_uncertainty_intervals(sample_means, sample_stds):
    """utils/posterior_predictive.py:30-46: the 2.5 % and 97.5 % points of the equal-weight Gaussian mixture of the draws' predictive
    densities, per test point; inputs (draws x test points), returns (lower, upper).  The reference estimates them from 1000 random
    mixture draws; here the mixture CDF mean_j Phi((x - mu_j) / sd_j) is solved by bisection, which is deterministic."""
    mu = np.asarray(sample_means, dtype=np.float64)
    sd = np.asarray(sample_stds, dtype=np.float64)
    if mu.ndim == 1:
        mu, sd = mu[:, None], sd[:, None]
    erf = np.vectorize(math.erf, otypes=[np.float64])

    def cdf(x):
        return np.mean(0.5 * (1.0 + erf((x[None, :] - mu) / (sd * math.sqrt(2.0)))), axis=0)

    out = []
    for p in (0.025, 0.975):
        lo, hi = np.min(mu - 10.0 * sd, axis=0), np.max(mu + 10.0 * sd, axis=0)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            below = cdf(mid) < p
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        out.append(0.5 * (lo + hi))
    return out[0], out[1]
