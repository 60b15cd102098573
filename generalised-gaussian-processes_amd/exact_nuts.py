"""Batched NUTS over the exact GP marginal likelihood on top of ``engine.exact_nuts_batch``: the Bayesian half of the reference's
hyper-parameter identification study (models/gpr_hmc.py on each of the data sets of experiments/hyperparameter_identification.py).

B data sets x ``chains`` chains run as independent workgroups of one device-resident sampler (csrc/sgp_exact_nuts.hip); the density is
``targets.ExactHmcTarget``'s.  torch is plumbing: starts are drawn and checked here (one value-only ``exact_eval_batch`` per round), the
chains themselves never visit the host.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .hmc import SplitMix, Trace, _trace_row
from .ml2 import MAX_D, MAX_N, _check_kernel, _dev, _engine
from .targets import in_range, theta_logp_and_grad

_GOLDEN, _MASK = 0x9E3779B97F4A7C15, (1 << 64) - 1
START_TRIES = 20  # hmc._find_start's


def _splitmix_output(seed: int, k: int) -> int:
    """The k-th output (k >= 1) of ``SplitMix(seed)``, without stepping through the k - 1 before it."""
    z = (int(seed) + k * _GOLDEN) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def chain_seed(seed: int, b: int, c: int) -> int:
    """The seed of chain c of data set b: the (c + 1)-th output of a ``SplitMix`` seeded with the (b + 1)-th output of
    ``SplitMix(seed)``.  It depends on (seed, b, c) alone -- not on how many data sets or chains the call has."""
    return _splitmix_output(_splitmix_output(seed, b + 1), c + 1)


def constrain(q):
    """exp of a position [log ls_1..d | log sig_f | log sig_n] as ``hmc._trace_row`` takes it."""
    v = np.exp(np.asarray(q, dtype=np.float64))
    return {"ls": v[:-2], "sig_f": float(v[-2]), "sig_n": float(v[-1])}


def _host(a):
    return np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def _host_sets(X, Y, Z=None, limits=(MAX_N, MAX_D, None)):
    """The host intake every batched sampler and mixture predictive shares: X, Y (and Z) as float64 numpy, Y lifted to B x N, a 1-D X
    or Z to one column, checked against ``limits`` = (max N, max d, max M).  Returns (Xh, Yh, Zh or None, B, N, d)."""
    Xh, Yh, Zh = _host(X), _host(Y), None if Z is None else _host(Z)
    Yh = Yh[None] if Yh.ndim == 1 else Yh
    Xh = Xh[:, None] if Xh.ndim == 1 else Xh
    B, N = Yh.shape
    d = Xh.shape[-1]
    if not 1 <= N <= limits[0] or not 1 <= d <= limits[1] or Xh.shape[-2] != N or (Xh.ndim != 2 and Xh.shape[0] != B):
        raise ValueError("X must be N x d or B x N x d with 1 <= N <= %d, 1 <= d <= %d, Y B x N (got X %s, Y %s)"
                         % (limits[0], limits[1], Xh.shape, Yh.shape))
    if Zh is not None:
        Zh = Zh[:, None] if Zh.ndim == 1 else Zh
        if not 1 <= Zh.shape[-2] <= limits[2] or Zh.shape[-1] != d or (Zh.ndim != 2 and Zh.shape[0] != B):
            raise ValueError("Z must be M x %d or %d x M x %d with 1 <= M <= %d (got %s)" % (d, B, d, limits[2], Zh.shape))
    return Xh, Yh, Zh, B, N, d


def _density(q, evaluate, noise_jitter=0.0, want_grad=False):
    """The theta density (``targets.theta_logp_and_grad``) at the rows of q (P x (d + 2), host): ``evaluate(theta)`` gives (F [P],
    gradient rows [P, d + 2] or None, info [P]) of ONE launch at theta = [exp | exp^2 | exp^2 + noise_jitter].  Returns (logp [P],
    grad [P, d + 2] or None) as numpy; a position out of range, a failed factorisation or a non-finite value gives -inf (and a zero
    gradient row)."""
    q = np.asarray(q, dtype=np.float64)
    P, nd = q.shape
    d = nd - 2
    ok = np.array([in_range(row) for row in q.tolist()])
    v = np.exp(np.where(ok[:, None], q, 0.0))
    F, g, info = evaluate(np.concatenate([v[:, :d], v[:, d:d + 1] ** 2, v[:, d + 1:] ** 2 + noise_jitter], 1))
    F, info = F.cpu().numpy(), info.cpu().numpy()
    g = g.cpu().numpy() if want_grad else None
    logp = np.full(P, -math.inf)
    grad = np.zeros((P, nd)) if want_grad else None
    for p in range(P):
        if not ok[p] or info[p] != 0 or not math.isfinite(F[p]):
            continue
        th, vs = q[p].tolist(), v[p].tolist()
        if want_grad:
            gp = g[p].tolist()
            logp[p], gr = theta_logp_and_grad(th, vs[:d], vs[d], vs[d + 1], float(F[p]), gp[:d], gp[d], gp[d + 1], finite_grad=True)
            grad[p] = gr
        else:
            logp[p] = theta_logp_and_grad(th, vs[:d], vs[d], vs[d + 1], float(F[p]))[0]
    return logp, grad


def logp_batch(engine, X, Y, q, ix, iy, kernel="rbf", jitter=0.0, want_grad=False):
    """``ExactHmcTarget``'s density at the rows of q (P x (d + 2), host) in ONE ``exact_eval_batch`` launch: row p on data set ix[p],
    target iy[p] (X, Y on the engine's device).  Returns (logp [P], grad [P, d + 2] or None) as numpy; a position out of range, a failed
    factorisation or a non-finite value gives -inf (and a zero gradient row)."""
    def evaluate(theta):
        F, _, g, info = engine.exact_eval_batch(X, Y, _dev(theta, engine), ix=ix, iy=iy, kernel=kernel, want_grad=want_grad)
        return F, g, info
    return _density(q, evaluate, jitter, want_grad)


@dataclass
class NutsBatchResult:
    """What a batched sampler returns (numpy).  Positions are unconstrained: [log ls_1..d | log sig_f | log sig_n]."""
    traces: list             # [B][chains] hmc.Trace, the surface sample_nuts_device gives
    samples: np.ndarray      # B x chains x n_samples x (d + 2)
    stats: np.ndarray        # B x chains x n_samples x 8: step_size, tree_size, depth, mean_tree_accept, diverging, energy, logp, evaluations so far
    seconds: np.ndarray      # B x chains x n_samples: device seconds per draw
    evaluations: np.ndarray  # B x chains
    draws: np.ndarray        # B x chains: draws finished, tuning included
    info: np.ndarray         # B x chains: 0, or the library's *_NUTS_BAD_START (no finite density at the start; that chain's rows are NaN)
    seeds: np.ndarray        # B x chains uint64: every chain's own seed (chain_seed)
    starts: np.ndarray       # B x chains x (d + 2)
    launches: int            # bounded launches the run took
    wall_clock_secs: float
    # what the draws were sampled with (the sampling frame fills them in): ``predict`` needs them
    X: Optional[np.ndarray] = None       # N x d or B x N x d
    Y: Optional[np.ndarray] = None       # B x N
    kernel: Optional[str] = None
    jitter: Optional[float] = None
    engine: object = None

    def _thinned(self, thin, fields: tuple, fn: str):
        """Every ``thin``-th draw of every chain as B x S x (d + 2), for the predictive ``fn`` that takes the data ``fields``."""
        data = ", ".join(fields)
        if any(getattr(self, name) is None for name in fields + ("kernel",)):
            raise ValueError("this result does not carry the data it was sampled with (%s, kernel, jitter): "
                             "use %s(%s, samples, X_test, ...)" % (data, fn, data))
        if int(thin) < 1:
            raise ValueError("thin >= 1 (got %r)" % (thin,))
        B, nd = self.samples.shape[0], self.samples.shape[-1]
        return self.samples[:, :, ::int(thin)].reshape(B, -1, nd)

    def posterior_mean(self):
        """B x (d + 2): the mean position of every data set over its chains and draws (NaN rows of bad chains left out)."""
        with np.errstate(invalid="ignore"):
            return np.nanmean(self.samples, axis=(1, 2))


@dataclass
class ExactNutsResult(NutsBatchResult):
    """``sample_exact_nuts_batch``'s result."""

    def predict(self, X_test, Y_test=None, thin=1, pred_noise=True, probs=None):
        """The mixture predictive (``exact_predict.predict_exact_batch``) over every ``thin``-th draw of every chain of each data set;
        ``probs``: the mixture's quantiles and PIT as well."""
        draws = self._thinned(thin, ("X", "Y"), "predict_exact_batch")
        from .exact_predict import predict_exact_batch
        return predict_exact_batch(self.X, self.Y, draws, X_test, Y_test, kernel=self.kernel, jitter=self.jitter or 0.0,
                                   pred_noise=pred_noise, engine=self.engine, probs=probs)


def _trace(samples, stats, seconds, evaluations, wall):
    rows = [_trace_row(constrain(row), row) for row in samples]
    st = {"step_size": stats[:, 0], "tree_size": stats[:, 1], "depth": stats[:, 2], "mean_tree_accept": stats[:, 3],
          "diverging": stats[:, 4] != 0.0, "energy": stats[:, 5], "logp": stats[:, 6], "perf_counter_diff": seconds}
    tr = Trace(rows, st)
    tr.n_leapfrog = int(evaluations)
    tr.wall_clock_secs = wall
    tr.device_resident = True
    return tr


def _sample_frame(result, logp, run, X, Y, Z, limits, n_samples, tune, chains, kernel, seed, start, seeds, jitter, engine):
    """What the batched samplers share: the host intake, the seeds (``chain_seed``, or ``seeds``), the set indices, the starts (checked
    with ``logp(eng, data, q0, idx)`` and redrawn chain by chain from the chain's own ``SplitMix``), the timed ``run(eng, data, q0,
    states, idx)`` -- the engine's sampler -- and the reshape into ``result``.  ``data`` is (X, Y[, Z]) on the device and ``idx`` the
    matching (ix, iy[, iz])."""
    _check_kernel(kernel)
    eng = _engine(engine)
    Xh, Yh, Zh, B, N, d = _host_sets(X, Y, Z, limits)
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
    held = [h for h in (Xh, Yh, Zh) if h is not None]
    idx = tuple(iy if h is Yh or h.ndim != 2 else None for h in held)  # a shared X or Z is set 0 for every chain
    data = tuple(_dev(h, eng) for h in held)
    base = np.asarray([math.log(2.0)] * d + [0.0, 0.0])
    if start is None:
        q0 = np.stack([base + r.uniform(-1.0, 1.0, nd) for r in rngs])
        for _ in range(START_TRIES):
            bad = np.flatnonzero(~np.isfinite(logp(eng, data, q0, idx)))
            if bad.size == 0:
                break
            for c in bad:
                q0[c] = base + rngs[c].uniform(-1.0, 1.0, nd)
    else:
        q0 = np.ascontiguousarray(np.broadcast_to(np.asarray(start, dtype=np.float64), (B, chains, nd))).reshape(C, nd)
    t0 = time.perf_counter()
    r = run(eng, data, _dev(q0, eng), [g.s for g in rngs], idx)
    wall = time.perf_counter() - t0
    host = {k: np.asarray(v) for k, v in r.items() if k != "launches"}
    samples, stats, seconds = host["samples"], host["stats"], host["seconds"]
    traces = [[_trace(samples[b * chains + c], stats[b * chains + c], seconds[b * chains + c], host["evaluations"][b * chains + c], wall)
               for c in range(chains)] for b in range(B)]
    sampled_with = dict(X=Xh, Y=Yh, kernel=kernel, jitter=float(jitter), engine=eng, **({} if Zh is None else {"Z": Zh}))
    return result(traces=traces, samples=samples.reshape(B, chains, n_samples, nd), stats=stats.reshape(B, chains, n_samples, -1),
                  seconds=seconds.reshape(B, chains, n_samples), evaluations=host["evaluations"].reshape(B, chains),
                  draws=host["draws"].reshape(B, chains), info=host["info"].reshape(B, chains), seeds=seeds,
                  starts=q0.reshape(B, chains, nd), launches=int(r["launches"]), wall_clock_secs=wall, **sampled_with)


def sample_exact_nuts_batch(X, Y, n_samples: int, tune: int, chains: int = 1, kernel="rbf", seed=None, start=None, seeds=None,
                            jitter=0.0, max_treedepth=10, step_scale=0.25, target_accept=0.8, evals_per_launch=None,
                            engine=None) -> ExactNutsResult:
    """``pm.sample(n_samples, tune=tune, chains=chains)`` over the exact GP of each of B data sets, all B x chains chains in one
    device-resident batch (one workgroup per chain; N <= 128, d <= 8, stationary kernels).

    X: N x d (shared) or B x N x d;  Y: B x N (or N).  Chain (b, c) has a seed of its own, ``chain_seed(seed, b, c)`` (``seed=None``:
    fresh entropy) -- or ``seeds[b][c]`` where ``seeds`` (B x chains) is given: a chain run alone with its seed (``result.seeds``) gives
    the bits it gives inside any batch.  Starts are ``hmc._find_start``'s: PyMC3's test point plus U(-1, 1) jitter from the chain's own
    ``SplitMix``; all chains are checked in one value-only launch and those with zero density redrawn, up to 20 times.  ``start`` ((d + 2)
    or B x chains x (d + 2)) is never replaced.  A chain whose start has no finite density is reported in ``info`` (its rows are NaN);
    nothing is raised."""
    return _sample_frame(
        ExactNutsResult, lambda eng, data, q0, idx: logp_batch(eng, *data, q0, *idx, kernel, jitter)[0],
        lambda eng, data, q0, states, idx: eng.exact_nuts_batch(
            *data, q0, states, tune, n_samples, ix=idx[0], iy=idx[1], kernel=kernel, jitter=jitter, max_treedepth=max_treedepth,
            step_scale=step_scale, target_accept=target_accept, evals_per_launch=evals_per_launch),
        X, Y, None, (MAX_N, MAX_D, None), n_samples, tune, chains, kernel, seed, start, seeds, jitter, engine)
