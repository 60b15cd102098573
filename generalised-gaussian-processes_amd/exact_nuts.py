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


def logp_batch(engine, X, Y, q, ix, iy, kernel="rbf", jitter=0.0, want_grad=False):
    """``ExactHmcTarget``'s density at the rows of q (P x (d + 2), host) in ONE ``exact_eval_batch`` launch: row p on data set ix[p],
    target iy[p] (X, Y on the engine's device).  Returns (logp [P], grad [P, d + 2] or None) as numpy; a position out of range, a failed
    factorisation or a non-finite value gives -inf (and a zero gradient row)."""
    q = np.asarray(q, dtype=np.float64)
    P, nd = q.shape
    d = nd - 2
    ok = np.array([in_range(row) for row in q.tolist()])
    v = np.exp(np.where(ok[:, None], q, 0.0))
    theta = np.concatenate([v[:, :d], v[:, d:d + 1] ** 2, v[:, d + 1:] ** 2 + jitter], 1)
    F, _, g, info = engine.exact_eval_batch(X, Y, _dev(theta, engine), ix=ix, iy=iy, kernel=kernel, want_grad=want_grad)
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


@dataclass
class ExactNutsResult:
    """``sample_exact_nuts_batch``'s result (numpy).  Positions are unconstrained: [log ls_1..d | log sig_f | log sig_n]."""
    traces: list             # [B][chains] hmc.Trace, the surface sample_nuts_device gives
    samples: np.ndarray      # B x chains x n_samples x (d + 2)
    stats: np.ndarray        # B x chains x n_samples x 8: step_size, tree_size, depth, mean_tree_accept, diverging, energy, logp, evaluations so far
    seconds: np.ndarray      # B x chains x n_samples: device seconds per draw
    evaluations: np.ndarray  # B x chains
    draws: np.ndarray        # B x chains: draws finished, tuning included
    info: np.ndarray         # B x chains: 0, or _lib.EXACT_NUTS_BAD_START (no finite density at the start; that chain's rows are NaN)
    seeds: np.ndarray        # B x chains uint64: every chain's own seed (chain_seed)
    starts: np.ndarray       # B x chains x (d + 2)
    launches: int            # bounded launches the run took
    wall_clock_secs: float
    # what the draws were sampled with (``sample_exact_nuts_batch`` fills them in): ``predict`` needs them
    X: Optional[np.ndarray] = None       # N x d or B x N x d
    Y: Optional[np.ndarray] = None       # B x N
    kernel: Optional[str] = None
    jitter: Optional[float] = None
    engine: object = None

    def predict(self, X_test, Y_test=None, thin=1, pred_noise=True):
        """The mixture predictive (``exact_predict.predict_exact_batch``) over every ``thin``-th draw of every chain of each data set."""
        if self.X is None or self.Y is None or self.kernel is None:
            raise ValueError("this result does not carry the data it was sampled with (X, Y, kernel, jitter): "
                             "use predict_exact_batch(X, Y, samples, X_test, ...)")
        if int(thin) < 1:
            raise ValueError("thin >= 1 (got %r)" % (thin,))
        from .exact_predict import predict_exact_batch
        B, nd = self.samples.shape[0], self.samples.shape[-1]
        draws = self.samples[:, :, ::int(thin)].reshape(B, -1, nd)
        return predict_exact_batch(self.X, self.Y, draws, X_test, Y_test, kernel=self.kernel, jitter=self.jitter or 0.0,
                                   pred_noise=pred_noise, engine=self.engine)

    def posterior_mean(self):
        """B x (d + 2): the mean position of every data set over its chains and draws (NaN rows of bad chains left out)."""
        with np.errstate(invalid="ignore"):
            return np.nanmean(self.samples, axis=(1, 2))


def _trace(samples, stats, seconds, evaluations, wall):
    rows = [_trace_row(constrain(row), row) for row in samples]
    st = {"step_size": stats[:, 0], "tree_size": stats[:, 1], "depth": stats[:, 2], "mean_tree_accept": stats[:, 3],
          "diverging": stats[:, 4] != 0.0, "energy": stats[:, 5], "logp": stats[:, 6], "perf_counter_diff": seconds}
    tr = Trace(rows, st)
    tr.n_leapfrog = int(evaluations)
    tr.wall_clock_secs = wall
    tr.device_resident = True
    return tr


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
    _check_kernel(kernel)
    eng = _engine(engine)
    Xh = np.asarray(X.cpu() if isinstance(X, torch.Tensor) else X, dtype=np.float64)
    Yh = np.asarray(Y.cpu() if isinstance(Y, torch.Tensor) else Y, dtype=np.float64)
    Yh = Yh[None] if Yh.ndim == 1 else Yh
    if Xh.ndim == 1:
        Xh = Xh[:, None]
    shared_x = Xh.ndim == 2
    B, N = Yh.shape
    d = Xh.shape[-1]
    if not 1 <= N <= MAX_N or not 1 <= d <= MAX_D or Xh.shape[-2] != N or (not shared_x and Xh.shape[0] != B):
        raise ValueError("X must be N x d or B x N x d with 1 <= N <= %d, 1 <= d <= %d, Y B x N (got X %s, Y %s)"
                         % (MAX_N, MAX_D, Xh.shape, Yh.shape))
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
    ix = None if shared_x else iy
    Xd, Yd = _dev(Xh, eng), _dev(Yh, eng)
    base = np.asarray([math.log(2.0)] * d + [0.0, 0.0])
    if start is None:
        q0 = np.stack([base + r.uniform(-1.0, 1.0, nd) for r in rngs])
        for _ in range(START_TRIES):
            bad = np.flatnonzero(~np.isfinite(logp_batch(eng, Xd, Yd, q0, ix, iy, kernel, jitter)[0]))
            if bad.size == 0:
                break
            for c in bad:
                q0[c] = base + rngs[c].uniform(-1.0, 1.0, nd)
    else:
        q0 = np.ascontiguousarray(np.broadcast_to(np.asarray(start, dtype=np.float64), (B, chains, nd))).reshape(C, nd)
    t0 = time.perf_counter()
    r = eng.exact_nuts_batch(Xd, Yd, _dev(q0, eng), [g.s for g in rngs], tune, n_samples, ix=ix, iy=iy, kernel=kernel, jitter=jitter,
                             max_treedepth=max_treedepth, step_scale=step_scale, target_accept=target_accept,
                             evals_per_launch=evals_per_launch)
    wall = time.perf_counter() - t0
    host = {k: np.asarray(v) for k, v in r.items() if k != "launches"}
    samples, stats, seconds = host["samples"], host["stats"], host["seconds"]
    traces = [[_trace(samples[b * chains + c], stats[b * chains + c], seconds[b * chains + c], host["evaluations"][b * chains + c], wall)
               for c in range(chains)] for b in range(B)]
    return ExactNutsResult(traces=traces, samples=samples.reshape(B, chains, n_samples, nd), stats=stats.reshape(B, chains, n_samples, -1),
                           seconds=seconds.reshape(B, chains, n_samples), evaluations=host["evaluations"].reshape(B, chains),
                           draws=host["draws"].reshape(B, chains), info=host["info"].reshape(B, chains), seeds=seeds,
                           starts=q0.reshape(B, chains, nd), launches=int(r["launches"]), wall_clock_secs=wall,
                           X=Xh, Y=Yh, kernel=kernel, jitter=float(jitter), engine=eng)
