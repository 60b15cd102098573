"""Test double for ``HipEngine.exact_nuts_batch`` on the CPU: per chain the Python sampler ``hmc.NUTS(rng=SplitMix(seed_c))`` -- whose
algorithm and random stream csrc/sgp_nuts.hpp follows line by line -- over ``exact_eval_batch`` (P = 1) + ``theta_logp_and_grad``.

TEST INFRASTRUCTURE ONLY.  With ``ExactNutsDouble()`` the evaluations are ``ExactBatchDouble``'s and ``sample_exact_nuts_batch``,
``GPR_HMC(device_sampler=True)`` and the experiment's ``--hmc`` run in the CPU suite; with ``ExactNutsDouble(evaluator=engine)`` they are
the device's ``exact_eval_batch``, which makes the double the host-driven chain the GPU tests hold the device-resident one against.
"""
import math
import time

import numpy as np
import torch

from exact_batch_double import ExactBatchDouble

from ggp_amd.hmc import NUTS, DiagMassAdapter, SplitMix
from ggp_amd.targets import in_range, theta_logp_and_grad

BAD_START = 1  # SGP_EXACT_NUTS_BAD_START


class ExactNutsDouble(ExactBatchDouble):
    def __init__(self, evaluator=None):
        super().__init__()
        self.calls.update(exact_nuts_batch=0)
        self.evaluator = evaluator if evaluator is not None else self
        if evaluator is not None:
            self.device = evaluator.device

    def logp_and_grad(self, Xc, yc, q, kernel="rbf", jitter=0.0):
        """ExactHmcTarget._eval with the batched entry point as the evaluation."""
        q = [float(v) for v in q]
        nd = len(q)
        d = nd - 2
        bad = (-math.inf, [0.0] * nd)
        if not in_range(q):
            return bad
        v = [math.exp(t) for t in q]
        theta = torch.tensor([v[:d] + [v[d] * v[d], v[d + 1] * v[d + 1] + jitter]], dtype=torch.float64).to(Xc.device)
        F, _, g, info = self.evaluator.exact_eval_batch(Xc, yc, theta, kernel=kernel)
        F, g, info = float(F.cpu()[0]), g.cpu()[0].tolist(), int(info.cpu()[0])
        if info != 0 or not math.isfinite(F):
            return bad
        return theta_logp_and_grad(q, v[:d], v[d], v[d + 1], F, g[:d], g[d], g[d + 1], finite_grad=True)

    def exact_nuts_batch(self, X, Y, q0, seeds, n_tune, n_draws, ix=None, iy=None, kernel="rbf", jitter=0.0, max_treedepth=10,
                         step_scale=0.25, target_accept=0.8, evals_per_launch=None):
        self.calls["exact_nuts_batch"] += 1
        X = X if X.dim() == 3 else X[None]
        Y = Y if Y.dim() == 2 else Y[None]
        N, d = X.shape[1], X.shape[2]
        if not 1 <= N <= 128 or not 1 <= d <= 8 or max_treedepth > 11 or kernel not in ("rbf", "matern32", "matern52"):
            raise ValueError("unsupported shape or kernel")
        q0 = np.asarray(q0.cpu() if isinstance(q0, torch.Tensor) else q0, dtype=np.float64).reshape(-1, d + 2)
        C, nd = q0.shape
        samples = np.full((C, n_draws, nd), np.nan)
        stats = np.full((C, n_draws, 8), np.nan)
        seconds = np.full((C, n_draws), np.nan)
        evaluations, draws, info = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int32)
        for c in range(C):
            Xc = X[0 if ix is None else int(ix[c])].contiguous()
            yc = Y[0 if iy is None else int(iy[c])].contiguous()
            nuts = NUTS(lambda q: self.logp_and_grad(Xc, yc, q, kernel, jitter), nd, step_scale=step_scale, target_accept=target_accept,
                        max_treedepth=max_treedepth, rng=SplitMix(int(seeds[c])))
            q = q0[c].copy()
            lp, g = nuts._eval(q)
            if not math.isfinite(lp):
                info[c], evaluations[c] = BAD_START, nuts.n_leapfrog
                continue
            nuts.mass = DiagMassAdapter(nd, initial_mean=q)
            for it in range(n_tune + n_draws):
                t0 = time.perf_counter()
                q, lp, g, st = nuts.draw(q, lp, g, it < n_tune)
                if it >= n_tune:
                    row = it - n_tune
                    samples[c, row] = q
                    stats[c, row] = [st["step_size"], st["tree_size"], st["depth"], st["mean_tree_accept"], float(st["diverging"]),
                                     st["energy"], lp, nuts.n_leapfrog]
                    seconds[c, row] = time.perf_counter() - t0
            evaluations[c], draws[c] = nuts.n_leapfrog, n_tune + n_draws
        t = torch.from_numpy
        return {"samples": t(samples), "stats": t(stats), "seconds": t(seconds), "evaluations": t(evaluations), "draws": t(draws),
                "info": t(info), "launches": 1}
