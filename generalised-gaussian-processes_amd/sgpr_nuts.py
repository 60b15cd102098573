"""Batched NUTS over the collapsed (VFE) sparse-GP bound at fixed inducing inputs on top of ``engine.vfe_nuts_batch``: the reference's
own model (models/bayesian_sgpr_hmc.py: ``train_fixed_model``, NUTS over theta = (ls, sig_f, sig_n) with Z fixed) for B data sets x
``chains`` chains at once.

All chains run as independent workgroups of one device-resident sampler (csrc/sgp_vfe_nuts.hip); the density is
``targets.HmcTarget``'s.  torch is plumbing: starts are drawn and checked here (one value-only ``vfe_eval_batch`` per round), the chains
themselves never visit the host.  Seeds, starts and traces are ``exact_nuts._sample_frame``'s, the frame of both batched samplers.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ._lib import VFE_BATCH_MAX_D as MAX_D, VFE_BATCH_MAX_M as MAX_M, VFE_BATCH_MAX_N as MAX_N
from .exact_nuts import NutsBatchResult, _density, _sample_frame
from .ml2 import _dev


def vfe_logp_batch(engine, X, Y, Z, q, ix, iy, iz, kernel="rbf", jitter=1e-6):
    """``HmcTarget``'s density at the rows of q (P x (d + 2), host) in ONE value-only ``vfe_eval_batch`` launch: row p on data set
    ix[p], target iy[p], inducing set iz[p] (X, Y, Z on the engine's device).  Returns logp [P] as numpy; a position out of range, a
    failed factorisation or a non-finite value gives -inf."""
    def evaluate(theta):
        out, _, info = engine.vfe_eval_batch(X, Y, Z, _dev(theta, engine), ix=ix, iy=iy, iz=iz, kernel=kernel, jitter=jitter, want_grad=False)
        return out[:, 0], None, info
    return _density(q, evaluate)[0]


@dataclass
class SgprNutsResult(NutsBatchResult):
    """``sample_sgpr_nuts_batch``'s result."""
    Z: Optional[np.ndarray] = None       # M x d or B x M x d

    def predict(self, X_test, Y_test=None, thin=1, pred_noise=True, probs=None):
        """The mixture predictive (``sgpr_predict.predict_sgpr_batch``) over every ``thin``-th draw of every chain of each data set, at
        the inducing inputs, kernel and jitter the draws were sampled with; ``probs``: the mixture's quantiles and PIT as well."""
        draws = self._thinned(thin, ("X", "Y", "Z"), "predict_sgpr_batch")
        from .sgpr_predict import predict_sgpr_batch
        return predict_sgpr_batch(self.X, self.Y, self.Z, draws, X_test, Y_test, kernel=self.kernel,
                                  jitter=1e-6 if self.jitter is None else self.jitter, pred_noise=pred_noise, engine=self.engine,
                                  probs=probs)

    def model(self, b: int):
        """A ``BayesianSparseGPR_HMC`` over data set b with its inducing inputs Z_b: ``mixture_posterior_predictive(model, X_test,
        traces[b][c])`` runs on it unchanged.  The class is the reference's RBF model, so the result must have been sampled with it."""
        from .gp_shim import GaussianLikelihood
        from .models import BayesianSparseGPR_HMC
        if self.X is None or self.Y is None or self.Z is None:
            raise ValueError("this result does not carry the data it was sampled with")
        if self.kernel != "rbf":
            raise ValueError("BayesianSparseGPR_HMC is the reference's RBF model (this result was sampled with %r)" % (self.kernel,))
        eng = self.engine if hasattr(self.engine, "suffstats") else None
        dev = eng.device if eng is not None else torch.device("cpu")
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
        return BayesianSparseGPR_HMC(t(self.X if self.X.ndim == 2 else self.X[b]), t(self.Y[b]), GaussianLikelihood(),
                                     t(self.Z if self.Z.ndim == 2 else self.Z[b]), engine=eng, jitter=self.jitter)


def sample_sgpr_nuts_batch(X, Y, Z, n_samples: int, tune: int, chains: int = 1, kernel="rbf", seed=None, start=None, seeds=None,
                           jitter=1e-6, max_treedepth=10, step_scale=0.25, target_accept=0.8, evals_per_launch=None,
                           engine=None) -> SgprNutsResult:
    """``pm.sample(n_samples, tune=tune, chains=chains)`` over theta of the collapsed sparse GP of each of B data sets at fixed
    inducing inputs, all B x chains chains in one device-resident batch (one workgroup per chain; M <= 64, N <= 65536, d <= 8,
    stationary kernels; ``jitter`` on K_uu).

    X: N x d (shared) or B x N x d;  Y: B x N (or N);  Z: M x d (shared) or B x M x d.  Chain (b, c) has a seed of its own,
    ``chain_seed(seed, b, c)`` (``seed=None``: fresh entropy) -- or ``seeds[b][c]`` where ``seeds`` (B x chains) is given: a chain run
    alone with its seed (``result.seeds``) gives the bits it gives inside any batch.  Starts are ``hmc._find_start``'s: PyMC3's test point
    plus U(-1, 1) jitter from the chain's own ``SplitMix``; all chains are checked in one value-only launch and those with zero density
    redrawn, up to 20 times.  ``start`` ((d + 2) or B x chains x (d + 2)) is never replaced.  A chain whose start has no finite density
    is reported in ``info`` (its rows are NaN); nothing is raised."""
    return _sample_frame(
        SgprNutsResult, lambda eng, data, q0, idx: vfe_logp_batch(eng, *data, q0, *idx, kernel, jitter),
        lambda eng, data, q0, states, idx: eng.vfe_nuts_batch(
            *data, q0, states, tune, n_samples, ix=idx[0], iy=idx[1], iz=idx[2], kernel=kernel, jitter=jitter,
            max_treedepth=max_treedepth, step_scale=step_scale, target_accept=target_accept, evals_per_launch=evals_per_launch),
        X, Y, Z, (MAX_N, MAX_D, MAX_M), n_samples, tune, chains, kernel, seed, start, seeds, jitter, engine)
