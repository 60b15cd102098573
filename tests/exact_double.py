"""Test double for the exact-GP entry points of HipEngine (``exact_eval`` / ``exact_predict``) in torch float64 on the CPU.

TEST INFRASTRUCTURE ONLY -- lets the CPU suite exercise ExactHmcTarget, GPR_HMC and the GPR branch of
full_mixture_posterior_predictive without a GPU, and is the yardstick the GPU tests compare the device against.  The
arithmetic is the textbook one (Rasmussen & Williams eq. 2.30 and 5.9): L = cholesky(A), alpha = A^-1 y by cholesky_solve,
dF/dtheta = 1/2 tr((alpha alpha^T - A^-1) dA/dtheta) with dA/dtheta written out analytically.
"""
import math

import torch

from fake_engine import KID, OracleEngine

LOG_2PI = math.log(2.0 * math.pi)


def kernel_parts(X1, X2, ls, sf2, kernel):
    """(K, h, D): K = sf2 k'(r2), h = dk'/dr2 (unit amplitude), D[q] = squared scaled differences of dimension q."""
    X1 = torch.as_tensor(X1, dtype=torch.float64)
    X2 = torch.as_tensor(X2, dtype=torch.float64)
    ls = torch.as_tensor(ls, dtype=torch.float64)
    diff = (X1[:, None, :] - X2[None, :, :]) / ls
    D = diff * diff
    r2 = D.sum(-1)
    kid = KID[kernel]
    if kid == 0:
        kp = torch.exp(-0.5 * r2)
        h = -0.5 * kp
    elif kid == 1:
        a = math.sqrt(3.0) * torch.sqrt(r2)
        e = torch.exp(-a)
        kp = (1.0 + a) * e
        h = -1.5 * e
    else:
        a = math.sqrt(5.0) * torch.sqrt(r2)
        e = torch.exp(-a)
        kp = (1.0 + a + a * a / 3.0) * e
        h = -(5.0 / 6.0) * (1.0 + a) * e
    return sf2 * kp, h, D


def exact_reference(X, y, ls, sf2, s2, kernel="rbf"):
    """dict(F, quad, logdet, trinv, g_ls, g_sf2, g_s2, info, L, alpha) in float64."""
    X = torch.as_tensor(X, dtype=torch.float64)
    y = torch.as_tensor(y, dtype=torch.float64).reshape(-1)
    N, d = X.shape
    lst = OracleEngine._ls(ls, d)
    K, h, D = kernel_parts(X, X, lst, float(sf2), kernel)
    A = K + float(s2) * torch.eye(N, dtype=torch.float64)
    L, info = torch.linalg.cholesky_ex(A)
    info = int(info)
    if info != 0:
        nan = float("nan")
        return {"F": nan, "info": info, "g_ls": torch.full((d,), nan, dtype=torch.float64), "g_sf2": nan, "g_s2": nan,
                "quad": nan, "logdet": nan, "trinv": nan, "L": L, "alpha": torch.full((N,), nan, dtype=torch.float64)}
    alpha = torch.cholesky_solve(y[:, None], L)[:, 0]
    Ainv = torch.cholesky_solve(torch.eye(N, dtype=torch.float64), L)
    quad = float(y @ alpha)
    logdet = 2.0 * float(torch.log(torch.diagonal(L)).sum())
    G = alpha[:, None] * alpha[None, :] - Ainv
    Gh = G * h
    g_ls = torch.stack([-float(sf2) / lst[q] * (Gh * D[:, :, q]).sum() for q in range(d)])
    g_sf2 = 0.5 * float((G * K).sum()) / float(sf2)
    g_s2 = 0.5 * (float(alpha @ alpha) - float(torch.diagonal(Ainv).sum()))
    return {"F": -0.5 * quad - 0.5 * logdet - 0.5 * N * LOG_2PI, "quad": quad, "logdet": logdet,
            "trinv": float(torch.diagonal(Ainv).sum()), "g_ls": g_ls, "g_sf2": g_sf2, "g_s2": g_s2, "info": info, "L": L,
            "alpha": alpha}


class ExactDouble(OracleEngine):
    """OracleEngine plus HipEngine's exact-GP surface.  ``factors`` is the pair (L, alpha), opaque to the callers as on the device."""

    def __init__(self):
        super().__init__()
        self.calls.update(exact_eval=0, exact_predict=0)

    def exact_eval(self, X, y, ls, sf2, s2, kernel="rbf", want_grad=True, want_factors=False):
        self.calls["exact_eval"] += 1
        r = exact_reference(X, y, ls, sf2, s2, kernel)
        res = {"F": r["F"], "out": [r["F"], r["quad"], r["logdet"], r["trinv"]], "info": r["info"]}
        if want_grad:
            res.update(ls=r["g_ls"].tolist(), sf2=r["g_sf2"], s2=r["g_s2"])
        if want_factors:
            res["factors"] = (r["L"], r["alpha"])
        return res

    def exact_predict(self, Xs, X, ls, sf2, s2, factors, kernel="rbf", pred_noise=True, full_cov=False):
        self.calls["exact_predict"] += 1
        L, alpha = factors
        d = X.shape[1]
        lst = self._ls(ls, d)
        Kxs = kernel_parts(X, Xs, lst, float(sf2), kernel)[0]
        V = torch.linalg.solve_triangular(L, Kxs, upper=False)
        mean = Kxs.T @ alpha
        var = float(sf2) - (V * V).sum(0) + (float(s2) if pred_noise else 0.0)
        cov = None
        if full_cov:
            cov = kernel_parts(Xs, Xs, lst, float(sf2), kernel)[0] - V.T @ V
            if pred_noise:
                cov = cov + float(s2) * torch.eye(Xs.shape[0], dtype=torch.float64)
        return mean, var, cov


def hand_logp(X, y, theta, kernel="rbf"):
    """The full log density of ExactHmcTarget written out by hand: exact marginal likelihood + Gamma(2, 1) on each ls,
    HalfCauchy(1) on sig_f and sig_n (log 2/pi - log(1 + x^2)), + the log-Jacobians sum(theta)."""
    theta = [float(v) for v in theta]
    d = len(theta) - 2
    ls = [math.exp(v) for v in theta[:d]]
    sf, sn = math.exp(theta[d]), math.exp(theta[d + 1])
    F = exact_reference(X, y, ls, sf * sf, sn * sn, kernel)["F"]
    lp = sum(math.log(l) - l for l in ls)  # Gamma(2, 1): log(l) - l - log Gamma(2) (= 0)
    lp += 2.0 * (math.log(2.0 / math.pi)) - math.log1p(sf * sf) - math.log1p(sn * sn)
    return F + lp + sum(theta)
