"""Test double for ``HipEngine.exact_eval_batch`` in torch float64 on the CPU: ``ExactDouble`` plus the batched entry point.

TEST INFRASTRUCTURE ONLY -- with it ``lml_surface``, ``fit_ml2`` and experiments/hyperparameter_identification.py run in the CPU
suite.  The arithmetic is the textbook one of tests/exact_double.py (Cholesky, cholesky_solve, the explicit inverse for the gradient),
batched over the P problems; it is itself held to TAU / 100 against tests/exact_batch_reference.py (tests/test_exact_batch.py).
"""
import math

import torch

from exact_double import LOG_2PI, ExactDouble
from fake_engine import KID


class ExactBatchDouble(ExactDouble):
    def __init__(self):
        super().__init__()
        self.calls.update(exact_eval_batch=0)

    def exact_eval_batch(self, X, Y, theta, ix=None, iy=None, kernel="rbf", want_grad=True):
        self.calls["exact_eval_batch"] += 1
        X = torch.as_tensor(X, dtype=torch.float64)
        Y = torch.as_tensor(Y, dtype=torch.float64)
        X = X if X.dim() == 3 else X[None]
        Y = Y if Y.dim() == 2 else Y[None]
        theta = torch.as_tensor(theta, dtype=torch.float64)
        P, N, d = theta.shape[0], X.shape[1], X.shape[2]
        if not 1 <= N <= 128 or not 1 <= d <= 8 or theta.shape[1] != d + 2 or KID[kernel] not in (0, 1, 2):
            raise ValueError("unsupported shape or kernel")
        zero = torch.zeros(P, dtype=torch.long)
        Xp = X[zero if ix is None else torch.as_tensor(ix).long()]
        yp = Y[zero if iy is None else torch.as_tensor(iy).long()]
        ls, sf2, s2 = theta[:, :d], theta[:, d], theta[:, d + 1]
        diff = (Xp[:, :, None, :] - Xp[:, None, :, :]) / ls[:, None, None, :]
        D = diff * diff
        r2 = D.sum(-1)
        kid = KID[kernel]
        if kid == 0:
            kp = torch.exp(-0.5 * r2)
            h = -0.5 * kp
        elif kid == 1:
            a = math.sqrt(3.0) * torch.sqrt(r2)
            e = torch.exp(-a)
            kp, h = (1.0 + a) * e, -1.5 * e
        else:
            a = math.sqrt(5.0) * torch.sqrt(r2)
            e = torch.exp(-a)
            kp, h = (1.0 + a + a * a / 3.0) * e, -(5.0 / 6.0) * (1.0 + a) * e
        eye = torch.eye(N, dtype=torch.float64)
        A = sf2[:, None, None] * kp + s2[:, None, None] * eye
        A = torch.where(torch.isfinite(A), A, torch.zeros_like(A))  # (a NaN theta: cholesky_ex must report, not raise)
        L, info = torch.linalg.cholesky_ex(A)
        info = info.to(torch.int32)
        info = torch.where(torch.isfinite(theta).all(1) & (theta > 0).all(1), info, torch.ones_like(info))
        ok = info == 0
        L = torch.where(ok[:, None, None], L, eye.expand(P, N, N))
        alpha = torch.cholesky_solve(yp[:, :, None], L)[:, :, 0]
        quad = (yp * alpha).sum(1)
        logdet = 2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)
        F = -0.5 * quad - 0.5 * logdet - 0.5 * N * LOG_2PI
        nan = torch.full((P,), float("nan"), dtype=torch.float64)
        out = torch.stack([F, quad, logdet, nan], 1)
        grads = None
        if want_grad:
            Ainv = torch.cholesky_solve(eye.expand(P, N, N), L)
            G = alpha[:, :, None] * alpha[:, None, :] - Ainv
            g_ls = -(sf2 / ls.T).T * ((G * h)[:, :, :, None] * D).sum((1, 2))
            g_sf2 = 0.5 * (G * kp).sum((1, 2))
            tr = torch.diagonal(Ainv, dim1=1, dim2=2).sum(1)
            g_s2 = 0.5 * ((alpha * alpha).sum(1) - tr)
            out[:, 3] = tr
            grads = torch.cat([g_ls, g_sf2[:, None], g_s2[:, None]], 1)
            grads[~ok] = float("nan")
        out[~ok] = float("nan")
        return out[:, 0], out, grads, info
