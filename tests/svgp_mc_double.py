"""CPU double of ``HipEngine.svgp_mc_elbo`` / ``svgp_mc_predict`` (the multi-class robust-max SVGP bound).

TEST INFRASTRUCTURE ONLY -- torch fp64 on the host, so that ``StochasticVariationalGP`` with a ``RobustMaxLikelihood`` trains and
predicts in a container without a GPU.  The forward restates include/sgp.h (the sgp_svgp_mc_elbo section) with ``lik_robustmax_pv`` of
csrc/sgp_lik.hpp -- the 20-point Gauss-Hermite sum, one variance per class, the floor 2^-40 sf2 -- and the gradients are torch
autograd's of that forward: independent of the closed-form reverse pass of tests/svgp_mc_reference.py and of the device code.  (The
Matern profiles keep r2 = 0 away from sqrt, so that autograd gives an even function's zero derivative there instead of NaN.)"""
import math

import torch

from fake_engine import KID, OracleEngine
from sgpmc_lik_double import GH_W, GH_X


def kern(X1, X2, ls, sf2, kid):
    D = X1[:, None, :] / ls - X2[None, :, :] / ls
    r2 = (D * D).sum(-1)
    if kid == 0:
        return sf2 * torch.exp(-0.5 * r2)
    pos = r2 > 0
    a = math.sqrt(3.0 if kid == 1 else 5.0) * torch.sqrt(torch.where(pos, r2, torch.ones_like(r2)))
    k = (1.0 + a) * torch.exp(-a) if kid == 1 else (1.0 + a + a * a / 3.0) * torch.exp(-a)
    return sf2 * torch.where(pos, k, torch.ones_like(r2))


def moments(X, Z, ls, sf2, m, LS, jitter, kid):
    """(MU, V): B x C latent means and variances (as formed) of the C classes; (L is returned for the status word)."""
    M = Z.shape[0]
    K = kern(Z, Z, ls, sf2, kid) + jitter * torch.eye(M, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    A = torch.linalg.solve_triangular(L, kern(Z, X, ls, sf2, kid), upper=False)      # M x B
    T = torch.einsum("cjm,jb->cmb", torch.tril(LS), A)                                # T_c = Ls_c^T A
    MU = A.T @ m.T
    V = sf2 - (A * A).sum(0)[:, None] + (T * T).sum(1).T
    return MU, V


def robustmax_pv_terms(y, MU, V, eps):
    """(ell (B), p (B)) under independent N(MU_bc, V_bc), V already floored; a label that is no integer of 0 .. C-1 gives NaN."""
    B, C = MU.shape
    ok = (y >= 0) & (y < C) & (y == torch.floor(y))
    yi = torch.where(ok, y, torch.zeros_like(y)).to(torch.int64)
    rows = torch.arange(B)
    sd = torch.sqrt(V)
    f = MU[rows, yi][:, None] + sd[rows, yi][:, None] * GH_X[None, :]                 # B x 20
    z = (f[:, :, None] - MU[:, None, :]) / sd[:, None, :]                             # B x 20 x C
    mask = torch.ones(B, C, dtype=torch.float64)
    mask[rows, yi] = 0.0
    p = (GH_W[None, :] * torch.exp((torch.special.log_ndtr(z) * mask[:, None, :]).sum(2))).sum(1)
    ell = p * math.log1p(-eps) + (1.0 - p) * math.log(eps / (C - 1))
    return torch.where(ok, ell, torch.full_like(ell, float("nan"))), p


def class_probs(MU, V, eps):
    """T x C predictive class probabilities by the same rule, one quadrature per class."""
    T, C = MU.shape
    cols = []
    for c in range(C):
        p = robustmax_pv_terms(torch.full((T,), float(c), dtype=torch.float64), MU, V, eps)[1]
        cols.append((1.0 - eps) * p + eps / (C - 1) * (1.0 - p))
    return torch.stack(cols, 1)


class SvgpMcOracleEngine(OracleEngine):
    def __init__(self):
        super().__init__()
        self.calls.update({"svgp_mc_elbo": 0, "svgp_mc_predict": 0})

    def svgp_mc_elbo(self, Xb, yb, Z, ls, sf2, m, LS, N_total, eps=1e-3, jitter=1e-6, kernel="rbf", with_grads=False):
        self.calls["svgp_mc_elbo"] += 1
        B, d = Xb.shape
        Cn, M = m.shape
        P = [t.detach().clone().requires_grad_(with_grads) for t in
             (self._ls(ls, d), torch.tensor(float(sf2), dtype=torch.float64), Z, m, LS)]
        lsv, s, Zv, mv, LSv = P
        with torch.enable_grad():
            MU, V = moments(Xb.detach(), Zv, lsv, s, mv, LSv, jitter, KID[kernel])
            floor = s.detach() * 2.0 ** -40
            ell, _ = robustmax_pv_terms(yb.detach(), MU, torch.where(V < floor, floor * torch.ones_like(V), V), float(eps))
            Ls = torch.tril(LSv)
            dg = torch.diagonal(Ls, dim1=1, dim2=2)
            kl = 0.5 * ((mv * mv).sum() + (Ls * Ls).sum() - Cn * M - 2.0 * torch.log(dg).sum())
            F = ell.sum() / B - kl / N_total
        res = {"out": torch.stack([F.detach(), ell.sum().detach(), kl.detach(), torch.zeros((), dtype=torch.float64)]),
               "info": torch.zeros(1, dtype=torch.int32)}
        if with_grads:
            g = torch.autograd.grad(F, P)
            res.update(g_ls=g[0], g_sf2=g[1].reshape(1), g_Z=g[2], g_m=g[3], g_LS=torch.tril(g[4]))
        return res

    def svgp_mc_predict(self, Xs, Z, ls, sf2, m, LS, eps=1e-3, jitter=1e-6, kernel="rbf", want_probs=True):
        self.calls["svgp_mc_predict"] += 1
        with torch.no_grad():
            s = torch.tensor(float(sf2), dtype=torch.float64)
            MU, V = moments(Xs, Z, self._ls(ls, Z.shape[1]), s, m, LS, jitter, KID[kernel])
            probs = class_probs(MU, torch.clamp(V, min=float(sf2) * 2.0 ** -40), float(eps)) if want_probs else None
        return MU, V, probs, torch.zeros(1, dtype=torch.int32)
