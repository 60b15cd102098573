"""Test double for ``HipEngine.vfe_predict_batch`` (and, inherited, ``exact_mixture``) in float64 on the CPU, on top of
``ExactPredictDouble`` and ``VfeNutsDouble``: with it ``predict_sgpr_batch``, ``SgprNutsResult.predict``, ``SgprBatchResult.predict`` and
the experiment's ``--sparse M --holdout K [--hmc]`` run in the CPU suite.

TEST INFRASTRUCTURE ONLY.  The predictive is ``vfe_predict_reference.predictive`` in float64 with triangular solves (the order the
kernel works in), problem by problem; ``bound`` is the F of ``VfeBatchDouble.vfe_eval_batch`` on the same problem, bit for bit, as the
device's is of ``sgp_vfe_eval_batch``.  The double is itself held to the long-double reference (tests/test_vfe_predict.py).
"""
import math

import numpy as np
import torch

import vfe_predict_reference as R
import vfe_reference as V
from exact_predict_double import ExactPredictDouble, _index
from fake_engine import KID
from vfe_nuts_double import VfeNutsDouble


class VfePredictDouble(ExactPredictDouble, VfeNutsDouble):
    """``fail`` as in ``VfeBatchDouble``: a callable (call number, problem) -> bool that forces ``info != 0``."""

    def __init__(self, fail=None):
        ExactPredictDouble.__init__(self)
        self.fail = fail
        self.calls.update(vfe_eval_batch=0, vfe_nuts_batch=0, vfe_predict_batch=0)

    def vfe_predict_batch(self, X, Y, Z, theta, Xs, ix=None, iy=None, iz=None, ixs=None, kernel="rbf", jitter=1e-6, pred_noise=True,
                          want_bound=True):
        call = self.calls["vfe_predict_batch"]
        self.calls["vfe_predict_batch"] += 1
        X, Y, Z, Xs, theta = (torch.as_tensor(a, dtype=torch.float64) for a in (X, Y, Z, Xs, theta))
        X = X if X.dim() == 3 else X[None]
        Y = Y if Y.dim() == 2 else Y[None]
        Z = Z if Z.dim() == 3 else Z[None]
        Xs = Xs if Xs.dim() == 3 else Xs[None]
        P, N, d, M, T = theta.shape[0], X.shape[1], X.shape[2], Z.shape[1], Xs.shape[1]
        if not 1 <= M <= 64 or not 1 <= N <= 65536 or not 1 <= d <= 8 or not 1 <= T <= 32768 or P < 1 or theta.shape[1] != d + 2 or \
                Z.shape[2] != d or Xs.shape[2] != d or Y.shape[1] != N or KID[kernel] not in (0, 1, 2):
            raise ValueError("unsupported shape or kernel")
        ix, iy = _index(ix, X.shape[0], P, "ix"), _index(iy, Y.shape[0], P, "iy")
        iz, ixs = _index(iz, Z.shape[0], P, "iz"), _index(ixs, Xs.shape[0], P, "ixs")
        mean = torch.full((P, T), math.nan, dtype=torch.float64)
        var = torch.full((P, T), math.nan, dtype=torch.float64)
        bound = torch.full((P,), math.nan, dtype=torch.float64) if want_bound else None
        info = torch.zeros(P, dtype=torch.int32)
        for p in range(P):
            th = theta[p].numpy()
            if not (np.isfinite(th) & (th > 0)).all() or (self.fail is not None and self.fail(call, p)):
                info[p] = 1
                continue
            Xp, yp, Zp = X[ix[p]].numpy(), Y[iy[p]].numpy(), Z[iz[p]].numpy()
            try:
                with np.errstate(all="ignore"):
                    # the kernel's gate on K_uu: a pivot at or below 8 M 2^-53 (sf2 + J) is rounding noise, not a pivot
                    K = V._stationary_k(Zp, Zp, th[:d], th[d], kernel, np.float64) + jitter * np.eye(M)
                    low = np.flatnonzero(np.diagonal(np.linalg.cholesky(K)) ** 2 <= 8.0 * M * 2.0 ** -53 * (th[d] + jitter))
                    if low.size:
                        info[p] = int(low[0]) + 1
                        continue
                    r, _ = R.predictive(Xp, yp, Zp, Xs[ixs[p]].numpy(), th[:d], th[d], th[d + 1], jitter, kernel, pred_noise, np.float64,
                                        "substitution")
                    F = V.stationary(Xp, yp, Zp, th[:d], th[d], th[d + 1], jitter, kernel, np.float64, "substitution", grads=False)[0]["F"]
            except np.linalg.LinAlgError:
                info[p] = 1
                continue
            if not np.isfinite(F):
                info[p] = 1
                continue
            mean[p], var[p] = torch.from_numpy(r["mean"]), torch.from_numpy(r["var"])
            if want_bound:
                bound[p] = float(F)
        return mean, var, bound, info
