"""Test double for ``HipEngine.vfe_nuts_batch`` on the CPU: per chain the Python sampler ``hmc.NUTS(rng=SplitMix(seed_c))`` -- whose
algorithm and random stream csrc/sgp_nuts.hpp follows line by line -- over ``vfe_eval_batch`` (P = 1) + ``theta_logp_and_grad``.

TEST INFRASTRUCTURE ONLY.  With ``VfeNutsDouble()`` the evaluations are ``VfeBatchDouble``'s and ``sample_sgpr_nuts_batch``,
``SgprBatchResult.sample_nuts`` and the experiment's ``--sparse M --hmc`` run in the CPU suite; with ``VfeNutsDouble(evaluator=engine)``
they are the device's ``vfe_eval_batch``, which makes the double the host-driven chain the GPU tests hold the device-resident one against.
"""
import math
import time

import numpy as np
import torch

from vfe_batch_double import VfeBatchDouble

from ggp_amd.hmc import NUTS, DiagMassAdapter, SplitMix
from ggp_amd.targets import in_range, theta_logp_and_grad

BAD_START = 1  # SGP_VFE_NUTS_BAD_START


class VfeNutsDouble(VfeBatchDouble):
    def __init__(self, evaluator=None, fail=None):
        super().__init__(fail=fail)
        self.calls.update(vfe_nuts_batch=0)
        self.evaluator = evaluator if evaluator is not None else self
        if evaluator is not None:
            self.device = evaluator.device

    def vfe_logp_and_grad(self, Xc, yc, Zc, q, kernel="rbf", jitter=1e-6):
        """HmcTarget's density with the batched entry point as the evaluation: the jitter goes to K_uu, not to the noise."""
        q = [float(v) for v in q]
        nd = len(q)
        d = nd - 2
        bad = (-math.inf, [0.0] * nd)
        if not in_range(q):
            return bad
        v = [math.exp(t) for t in q]
        theta = torch.tensor([v[:d] + [v[d] * v[d], v[d + 1] * v[d + 1]]], dtype=torch.float64).to(Xc.device)
        out, _, info = self.evaluator.vfe_eval_batch(Xc, yc, Zc, theta, kernel=kernel, jitter=jitter)
        row, info = out.cpu()[0].tolist(), int(info.cpu()[0])
        if info != 0 or not math.isfinite(row[0]):
            return bad
        return theta_logp_and_grad(q, v[:d], v[d], v[d + 1], row[0], row[1:1 + d], row[1 + d], row[2 + d], finite_grad=True)

    def vfe_nuts_batch(self, X, Y, Z, q0, seeds, n_tune, n_draws, ix=None, iy=None, iz=None, kernel="rbf", jitter=1e-6, max_treedepth=10,
                       step_scale=0.25, target_accept=0.8, evals_per_launch=None):
        self.calls["vfe_nuts_batch"] += 1
        X = X if X.dim() == 3 else X[None]
        Y = Y if Y.dim() == 2 else Y[None]
        Z = Z if Z.dim() == 3 else Z[None]
        N, d, M = X.shape[1], X.shape[2], Z.shape[1]
        if not 1 <= M <= 64 or not 1 <= N <= 65536 or not 1 <= d <= 8 or max_treedepth > 11 or kernel not in ("rbf", "matern32", "matern52"):
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
            Zc = Z[0 if iz is None else int(iz[c])].contiguous()
            nuts = NUTS(lambda q: self.vfe_logp_and_grad(Xc, yc, Zc, q, kernel, jitter), nd, step_scale=step_scale,
                        target_accept=target_accept, max_treedepth=max_treedepth, rng=SplitMix(int(seeds[c])))
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
