"""Test doubles for ``HipEngine.mixture_quantiles`` in float64 on the CPU, on top of ``ExactPredictDouble`` and ``VfePredictDouble``:
with them ``predict_*_batch(..., probs=...)``, the results' ``predict(..., probs=...)``, ``ggp_amd.mixture_quantiles`` and the
experiment's ``--calibration`` run in the CPU suite.

TEST INFRASTRUCTURE ONLY.  The quantile is a plain bisection of the tail sum (``torch.special.erfc``) over the interface's proven
bracket down to a fixed point of the midpoint: no Newton step, nothing of the kernel's code.  It is itself held to the acceptance rule
of tests/mixture_quantile_reference.py (tests/test_mixture_quantile.py)."""
import math

import numpy as np
import torch

from exact_predict_double import ExactPredictDouble
from vfe_predict_double import VfePredictDouble


def quantiles_numpy(mean, var, info, offsets, probs, Ytest=None):
    """(quantiles G x Q x T, pit G x T or None) in numpy."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    info = np.asarray(info).reshape(-1)
    P, T = mean.shape
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    G = off.size - 1
    pr = np.asarray(probs, dtype=np.float64).reshape(-1)
    if G < 1 or off[0] != 0 or off[-1] != P or np.any(np.diff(off) < 0):
        raise ValueError("offsets must be non-decreasing from 0 to %d" % P)
    if not 1 <= pr.size <= 8 or not np.all((pr >= 1e-9) & (pr <= 1.0 - 1e-9)):
        raise ValueError("probs must be 1 to 8 probabilities in [1e-9, 1 - 1e-9]")
    y = None if Ytest is None else np.asarray(Ytest, dtype=np.float64)
    if y is not None and y.shape != (G, T):
        raise ValueError("Ytest must be %d x %d" % (G, T))
    quant = np.full((G, pr.size, T), np.nan)
    pit = None if y is None else np.full((G, T), np.nan)
    upper = torch.from_numpy(pr > 0.5)[:, None, None]                                   # Q x 1 x 1
    pt = torch.from_numpy(np.where(pr > 0.5, 1.0 - pr, pr))[:, None]                    # Q x 1
    z = torch.sqrt(-2.0 * torch.log(pt))[:, None]                                       # Q x 1 x 1
    for g in range(G):
        keep = np.flatnonzero(info[off[g]:off[g + 1]] == 0) + off[g]
        if keep.size == 0:
            continue
        mu, v = torch.from_numpy(mean[keep]), torch.from_numpy(var[keep])               # n x T
        good = ((v > 0) & torch.isfinite(v) & torch.isfinite(mu)).all(0)                # T
        mu, sg = mu[:, good], torch.sqrt(v[:, good])
        if mu.shape[1] == 0:
            continue

        def tail(x, up):  # x: Q x T' -> Q x T'
            u = (x[:, None, :] - mu[None]) / (sg[None] * math.sqrt(2.0))
            return (0.5 * torch.special.erfc(torch.where(up, u, -u))).mean(1)
        lo = (mu[None] - z * sg[None]).min(1).values
        hi = (mu[None] + z * sg[None]).max(1).values
        for _ in range(2000):
            mid = lo + 0.5 * (hi - lo)
            if bool(((mid <= lo) | (mid >= hi)).all()):
                break
            t = tail(mid, upper)
            above = torch.where(upper[:, 0], t > pt, t < pt)
            lo, hi = torch.where(above, mid, lo), torch.where(above, hi, mid)
        col = np.flatnonzero(good.numpy())
        quant[g][:, col] = (lo + 0.5 * (hi - lo)).numpy()
        if y is not None:
            yy = torch.from_numpy(y[g][col])[None]
            pit[g, col] = tail(yy, torch.zeros(1, 1, 1, dtype=torch.bool))[0].numpy()
    return quant, pit


class _Quantiles:
    def mixture_quantiles(self, mean, var, info, offsets, probs, Ytest=None, want_iters=False):
        self.calls["mixture_quantiles"] = self.calls.get("mixture_quantiles", 0) + 1
        as_np = lambda a: a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
        quant, pit = quantiles_numpy(as_np(mean), as_np(var), as_np(info), offsets, probs, None if Ytest is None else as_np(Ytest))
        return {"quantiles": torch.from_numpy(quant), "pit": None if pit is None else torch.from_numpy(pit),
                "iters": torch.ones(quant.shape[0], quant.shape[2], dtype=torch.int32) if want_iters else None}


class ExactQuantileDouble(_Quantiles, ExactPredictDouble):
    def __init__(self, evaluator=None):
        super().__init__(evaluator)
        self.calls.update(mixture_quantiles=0)


class SgprQuantileDouble(_Quantiles, VfePredictDouble):
    def __init__(self, fail=None):
        VfePredictDouble.__init__(self, fail)
        self.calls.update(mixture_quantiles=0)
