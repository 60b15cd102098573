"""Test double for ``HipEngine.exact_predict_batch`` and ``HipEngine.exact_mixture`` in torch float64 on the CPU, on top of
``ExactNutsDouble``: with it ``predict_exact_batch``, ``ExactNutsResult.predict``, ``Ml2Result.predict`` and the experiment's
``--holdout`` run in the CPU suite.

TEST INFRASTRUCTURE ONLY.  The predictive is the device's algorithm in textbook form (Cholesky, the explicit L^-1, V = L^-1 K*, var =
sf2 - sum V^2 (+ s2), not clamped), problem by problem; the mixture is the kernel's formulas in numpy.  Both are themselves held to the
long-double reference of tests/exact_predict_reference.py (tests/test_exact_predict.py).
"""
import math

import numpy as np
import torch

from exact_double import kernel_parts
from exact_nuts_double import ExactNutsDouble
from fake_engine import KID


def _index(idx, n_sets, P, name):
    if idx is None:
        return np.zeros(P, dtype=np.int64)
    host = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx).reshape(-1)
    if host.size != P or (P and (host.min() < 0 or host.max() >= n_sets)):
        raise ValueError("%s must hold %d indices in [0, %d)" % (name, P, n_sets))
    return host.astype(np.int64)


class ExactPredictDouble(ExactNutsDouble):
    def __init__(self, evaluator=None):
        super().__init__(evaluator)
        self.calls.update(exact_predict_batch=0, exact_mixture=0)

    def exact_predict_batch(self, X, Y, theta, Xs, ix=None, iy=None, ixs=None, kernel="rbf", pred_noise=True):
        self.calls["exact_predict_batch"] += 1
        X, Y, Xs, theta = (torch.as_tensor(a, dtype=torch.float64) for a in (X, Y, Xs, theta))
        X = X if X.dim() == 3 else X[None]
        Y = Y if Y.dim() == 2 else Y[None]
        Xs = Xs if Xs.dim() == 3 else Xs[None]
        P, N, d, T = theta.shape[0], X.shape[1], X.shape[2], Xs.shape[1]
        if not 1 <= N <= 128 or not 1 <= d <= 8 or not 1 <= T <= 32768 or P < 1 or theta.shape[1] != d + 2 or Xs.shape[2] != d or \
                KID[kernel] not in (0, 1, 2):
            raise ValueError("unsupported shape or kernel")
        ix, iy, ixs = _index(ix, X.shape[0], P, "ix"), _index(iy, Y.shape[0], P, "iy"), _index(ixs, Xs.shape[0], P, "ixs")
        mean = torch.full((P, T), math.nan, dtype=torch.float64)
        var = torch.full((P, T), math.nan, dtype=torch.float64)
        info = torch.zeros(P, dtype=torch.int32)
        eye = torch.eye(N, dtype=torch.float64)
        for p in range(P):
            th = theta[p]
            if not bool((torch.isfinite(th) & (th > 0)).all()):
                info[p] = 1
                continue
            ls, sf2, s2 = th[:d], float(th[d]), float(th[d + 1])
            Xp = X[ix[p]]
            A = kernel_parts(Xp, Xp, ls, sf2, kernel)[0] + s2 * eye
            L, bad = torch.linalg.cholesky_ex(A)
            if int(bad) != 0:
                info[p] = int(bad)
                continue
            Linv = torch.linalg.solve_triangular(L, eye, upper=False)
            alpha = Linv.T @ (Linv @ Y[iy[p]])
            Ks = kernel_parts(Xp, Xs[ixs[p]], ls, sf2, kernel)[0]
            V = Linv @ Ks
            mean[p] = Ks.T @ alpha
            var[p] = sf2 - (V * V).sum(0) + (s2 if pred_noise else 0.0)
        return mean, var, info

    def exact_mixture(self, mean, var, info, offsets, Ytest=None):
        self.calls["exact_mixture"] += 1
        mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
        info = np.asarray(info).reshape(-1)
        P, T = mean.shape
        off = np.asarray(offsets, dtype=np.int64).reshape(-1)
        G = off.size - 1
        if G < 1 or off[0] != 0 or off[-1] != P or np.any(np.diff(off) < 0):
            raise ValueError("offsets must be non-decreasing from 0 to %d" % P)
        y = None if Ytest is None else np.asarray(Ytest, dtype=np.float64)
        if y is not None and y.shape != (G, T):
            raise ValueError("Ytest must be %d x %d" % (G, T))
        out = {k: np.full((G, T), np.nan) for k in ("mean", "var", "logpdf", "mean_logpdf")}
        kept = np.zeros(G, dtype=np.int32)
        for g in range(G):
            keep = np.flatnonzero(info[off[g]:off[g + 1]] == 0) + off[g]
            n = kept[g] = keep.size
            if n == 0:
                continue
            mu, v = mean[keep], var[keep]
            m = mu.sum(0) / n
            out["mean"][g] = m
            out["var"][g] = (v + (mu - m) ** 2).sum(0) / n
            if y is not None:
                with np.errstate(invalid="ignore", divide="ignore"):
                    l = -0.5 * np.log(2.0 * math.pi * v) - 0.5 * (y[g] - mu) ** 2 / v
                    mx = l.max(0)
                    out["logpdf"][g] = mx + np.log(np.exp(l - mx).sum(0) / n)
                out["mean_logpdf"][g] = l.sum(0) / n
        t = torch.from_numpy
        res = {"mean": t(out["mean"]), "var": t(out["var"]), "kept": t(kept), "logpdf": None, "mean_logpdf": None}
        if y is not None:
            res.update(logpdf=t(out["logpdf"]), mean_logpdf=t(out["mean_logpdf"]))
        return res
