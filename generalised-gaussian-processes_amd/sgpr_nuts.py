"""Batched NUTS over the collapsed (VFE) sparse-GP bound at fixed inducing inputs on top of ``engine.vfe_nuts_batch``: the reference's
own model (models/bayesian_sgpr_hmc.py: ``train_fixed_model``, NUTS over theta = (ls, sig_f, sig_n) with Z fixed) for B data sets x
``chains`` chains at once.

All chains run as independent workgroups of one device-resident sampler (csrc/sgp_vfe_nuts.hip); the density is
``targets.HmcTarget``'s.  torch is plumbing: starts are drawn and checked here (one value-only ``vfe_eval_batch`` per round), the chains
themselves never visit the host.  Seeds and starts are ``exact_nuts.sample_exact_nuts_batch``'s, rule for rule.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ._lib import VFE_BATCH_MAX_D as MAX_D, VFE_BATCH_MAX_M as MAX_M, VFE_BATCH_MAX_N as MAX_N
from .exact_nuts import START_TRIES, _trace, chain_seed
from .hmc import SplitMix
from .ml2 import _check_kernel, _dev, _engine
from .targets import in_range, theta_logp_and_grad


def vfe_logp_batch(engine, X, Y, Z, q, ix, iy, iz, kernel="rbf", jitter=1e-6):
    """``HmcTarget``'s density at the rows of q (P x (d + 2), host) in ONE value-only ``vfe_eval_batch`` launch: row p on data set
    ix[p], target iy[p], inducing set iz[p] (X, Y, Z on the engine's device).  Returns logp [P] as numpy; a position out of range, a
    failed factorisation or a non-finite value gives -inf."""
    q = np.asarray(q, dtype=np.float64)
    P, nd = q.shape
    d = nd - 2
    ok = np.array([in_range(row) for row in q.tolist()])
    v = np.exp(np.where(ok[:, None], q, 0.0))
    theta = np.concatenate([v[:, :d], v[:, d:d + 1] ** 2, v[:, d + 1:] ** 2], 1)
    out, _, info = engine.vfe_eval_batch(X, Y, Z, _dev(theta, engine), ix=ix, iy=iy, iz=iz, kernel=kernel, jitter=jitter, want_grad=False)
    F, info = out[:, 0].cpu().numpy(), info.cpu().numpy()
    logp = np.full(P, -math.inf)
    for p in range(P):
        if ok[p] and info[p] == 0 and math.isfinite(F[p]):
            vs = v[p].tolist()
            logp[p] = theta_logp_and_grad(q[p].tolist(), vs[:d], vs[d], vs[d + 1], float(F[p]))[0]
    return logp


@dataclass
class SgprNutsResult:
    """``sample_sgpr_nuts_batch``'s result (numpy).  Positions are unconstrained: [log ls_1..d | log sig_f | log sig_n]."""
    traces: list             # [B][chains] hmc.Trace, the surface sample_nuts_device gives
    samples: np.ndarray      # B x chains x n_samples x (d + 2)
    stats: np.ndarray        # B x chains x n_samples x 8: step_size, tree_size, depth, mean_tree_accept, diverging, energy, logp, evaluations so far
    seconds: np.ndarray      # B x chains x n_samples: device seconds per draw
    evaluations: np.ndarray  # B x chains
    draws: np.ndarray        # B x chains: draws finished, tuning included
    info: np.ndarray         # B x chains: 0, or _lib.VFE_NUTS_BAD_START (no finite density at the start; that chain's rows are NaN)
    seeds: np.ndarray        # B x chains uint64: every chain's own seed (chain_seed)
    starts: np.ndarray       # B x chains x (d + 2)
    launches: int            # bounded launches the run took
    wall_clock_secs: float
    # what the draws were sampled with
    X: Optional[np.ndarray] = None       # N x d or B x N x d
    Y: Optional[np.ndarray] = None       # B x N
    Z: Optional[np.ndarray] = None       # M x d or B x M x d
    kernel: Optional[str] = None
    jitter: Optional[float] = None
    engine: object = None

    def posterior_mean(self):
        """B x (d + 2): the mean position of every data set over its chains and draws (NaN rows of bad chains left out)."""
        with np.errstate(invalid="ignore"):
            return np.nanmean(self.samples, axis=(1, 2))

    def predict(self, X_test, Y_test=None, thin=1, pred_noise=True):
        """The mixture predictive (``sgpr_predict.predict_sgpr_batch``) over every ``thin``-th draw of every chain of each data set, at
        the inducing inputs, kernel and jitter the draws were sampled with."""
        if self.X is None or self.Y is None or self.Z is None or self.kernel is None:
            raise ValueError("this result does not carry the data it was sampled with (X, Y, Z, kernel, jitter): "
                             "use predict_sgpr_batch(X, Y, Z, samples, X_test, ...)")
        if int(thin) < 1:
            raise ValueError("thin >= 1 (got %r)" % (thin,))
        from .sgpr_predict import predict_sgpr_batch
        B, nd = self.samples.shape[0], self.samples.shape[-1]
        draws = self.samples[:, :, ::int(thin)].reshape(B, -1, nd)
        return predict_sgpr_batch(self.X, self.Y, self.Z, draws, X_test, Y_test, kernel=self.kernel,
                                  jitter=1e-6 if self.jitter is None else self.jitter, pred_noise=pred_noise, engine=self.engine)

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
    _check_kernel(kernel)
    eng = _engine(engine)
    Xh = np.asarray(X.cpu() if isinstance(X, torch.Tensor) else X, dtype=np.float64)
    Yh = np.asarray(Y.cpu() if isinstance(Y, torch.Tensor) else Y, dtype=np.float64)
    Zh = np.asarray(Z.cpu() if isinstance(Z, torch.Tensor) else Z, dtype=np.float64)
    Yh = Yh[None] if Yh.ndim == 1 else Yh
    if Xh.ndim == 1:
        Xh = Xh[:, None]
    if Zh.ndim == 1:
        Zh = Zh[:, None]
    shared_x, shared_z = Xh.ndim == 2, Zh.ndim == 2
    B, N = Yh.shape
    d, M = Xh.shape[-1], Zh.shape[-2]
    if not 1 <= N <= MAX_N or not 1 <= d <= MAX_D or Xh.shape[-2] != N or (not shared_x and Xh.shape[0] != B):
        raise ValueError("X must be N x d or B x N x d with 1 <= N <= %d, 1 <= d <= %d, Y B x N (got X %s, Y %s)"
                         % (MAX_N, MAX_D, Xh.shape, Yh.shape))
    if not 1 <= M <= MAX_M or Zh.shape[-1] != d or (not shared_z and Zh.shape[0] != B):
        raise ValueError("Z must be M x %d or %d x M x %d with 1 <= M <= %d (got %s)" % (d, B, d, MAX_M, Zh.shape))
    if chains < 1 or n_samples < 1 or tune < 0:
        raise ValueError("chains >= 1, n_samples >= 1, tune >= 0 (got %d, %d, %d)" % (chains, n_samples, tune))
    nd, C = d + 2, B * chains
    if seeds is None:
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0] >> 1)
        seeds = [[chain_seed(seed, b, c) for c in range(chains)] for b in range(B)]
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(B, chains)
    rngs = [SplitMix(int(s)) for s in seeds.reshape(-1)]
    iy = np.repeat(np.arange(B, dtype=np.int32), chains)
    ix, iz = None if shared_x else iy, None if shared_z else iy
    Xd, Yd, Zd = _dev(Xh, eng), _dev(Yh, eng), _dev(Zh, eng)
    base = np.asarray([math.log(2.0)] * d + [0.0, 0.0])
    if start is None:
        q0 = np.stack([base + r.uniform(-1.0, 1.0, nd) for r in rngs])
        for _ in range(START_TRIES):
            bad = np.flatnonzero(~np.isfinite(vfe_logp_batch(eng, Xd, Yd, Zd, q0, ix, iy, iz, kernel, jitter)))
            if bad.size == 0:
                break
            for c in bad:
                q0[c] = base + rngs[c].uniform(-1.0, 1.0, nd)
    else:
        q0 = np.ascontiguousarray(np.broadcast_to(np.asarray(start, dtype=np.float64), (B, chains, nd))).reshape(C, nd)
    t0 = time.perf_counter()
    r = eng.vfe_nuts_batch(Xd, Yd, Zd, _dev(q0, eng), [g.s for g in rngs], tune, n_samples, ix=ix, iy=iy, iz=iz, kernel=kernel,
                           jitter=jitter, max_treedepth=max_treedepth, step_scale=step_scale, target_accept=target_accept,
                           evals_per_launch=evals_per_launch)
    wall = time.perf_counter() - t0
    host = {k: np.asarray(v) for k, v in r.items() if k != "launches"}
    samples, stats, seconds = host["samples"], host["stats"], host["seconds"]
    traces = [[_trace(samples[b * chains + c], stats[b * chains + c], seconds[b * chains + c], host["evaluations"][b * chains + c], wall)
               for c in range(chains)] for b in range(B)]
    return SgprNutsResult(traces=traces, samples=samples.reshape(B, chains, n_samples, nd), stats=stats.reshape(B, chains, n_samples, -1),
                          seconds=seconds.reshape(B, chains, n_samples), evaluations=host["evaluations"].reshape(B, chains),
                          draws=host["draws"].reshape(B, chains), info=host["info"].reshape(B, chains), seeds=seeds,
                          starts=q0.reshape(B, chains, nd), launches=int(r["launches"]), wall_clock_secs=wall,
                          X=Xh, Y=Yh, Z=Zh, kernel=kernel, jitter=float(jitter), engine=eng)
