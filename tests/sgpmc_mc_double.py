"""CPU double of the engine for SGPMC with the multi-class robust-max likelihood: ``SgpmcLikOracleEngine`` + ``sgpmc_mc_rows`` /
``sgpmc_mc_tail``.

TEST INFRASTRUCTURE ONLY -- torch fp64 on the host, so that ``targets.SgpmcTarget(likelihood="multiclass")``, ``hmc.sample_hmc`` and
``sgp_hmc`` run in a container without a GPU.  The two methods restate include/sgp.h (sgp_sgpmc_mc_rows, sgp_sgpmc_mc_tail) with
``lik_robustmax`` of csrc/sgp_lik.hpp: the 20-point Gauss-Hermite sum and ITS derivatives, the variance floor 2^-40 sf2, dv of both signs.
``t_out`` is used as the HIP engine uses it -- T on return of a value-only call, the folded T_in = diag(dv) T - DMU V^T / (2 sf2) with the
adjoints -- and the factored pass 2 of the parent class takes whatever ``t_in`` it is handed."""
import math

import torch

from fake_engine import KID
from oracle import vfe_oracle as O
from sgpmc_lik_double import GH_W, GH_X, SgpmcLikOracleEngine


def robustmax_terms(y, MU, var, eps):
    """(ell (N), dMU (N x C), dvar (N), p (N)) as csrc/sgp_lik.hpp forms them; a label that is no integer of 0 .. C-1 gives NaN."""
    N, C = MU.shape
    ok = (y >= 0) & (y < C) & (y == torch.floor(y))
    yi = torch.where(ok, y, torch.zeros_like(y)).to(torch.int64)
    rows = torch.arange(N)
    sd = torch.sqrt(var)
    D = (MU[rows, yi][:, None] - MU) / sd[:, None]
    mask = torch.ones(N, C, dtype=torch.float64)
    mask[rows, yi] = 0.0
    z = GH_X[None, :, None] + D[:, None, :]
    lp = torch.special.log_ndtr(z)
    P = GH_W[None, :] * torch.exp((lp * mask[:, None, :]).sum(2))
    p = P.sum(1)
    r = torch.exp(-0.5 * z * z - 0.5 * math.log(2.0 * math.pi) - lp)
    R = (P[:, :, None] * r * mask[:, None, :]).sum(1)
    l1, l0 = math.log1p(-eps), math.log(eps / (C - 1))
    dD = (l1 - l0) * R
    dMU = -dD / sd[:, None]
    dMU[rows, yi] += dD.sum(1) / sd
    dvar = -(dD * D).sum(1) / (2.0 * var)
    ell = p * l1 + (1.0 - p) * l0
    nan = torch.full_like(ell, float("nan"))
    return torch.where(ok, ell, nan), torch.where(ok[:, None], dMU, nan[:, None]), torch.where(ok, dvar, nan), p


def class_probs(MU, var, eps):
    """(N x C) predictive class probabilities (1 - eps) P(c largest) + eps / (C - 1) (1 - P(c largest)) by the same 20-point rule."""
    N, C = MU.shape
    cols = []
    for c in range(C):
        p = robustmax_terms(torch.full((N,), float(c), dtype=torch.float64), MU, var, eps)[3]
        cols.append((1.0 - eps) * p + eps / (C - 1) * (1.0 - p))
    return torch.stack(cols, 1)


class SgpmcMcOracleEngine(SgpmcLikOracleEngine):
    def __init__(self):
        super().__init__()
        self.calls.update({"sgpmc_mc_rows": 0, "sgpmc_mc_tail": 0})

    def sgpmc_mc_rows(self, X, y, Z, ls, sf2, V, kuu_linv, t_out, kernel="rbf", eps=1e-3, want_adjoints=False, want_moments=False):
        self.calls["sgpmc_mc_rows"] += 1
        N, (M, d) = X.shape[0], Z.shape
        sf2 = float(sf2)
        T = O.kern(X, Z, self._ls(ls, d), 1.0, KID[kernel]) @ kuu_linv.T      # unit amplitude, N x M
        a = sf2 * T
        MU, var = a @ V.T, sf2 - (a * a).sum(1)
        res = {}
        if want_moments or y is None:
            res.update(mu=MU.T.contiguous(), var=var)
        if y is not None:
            floor = sf2 * 2.0 ** -40
            floored = var < floor
            ell, dMU, dv, _ = robustmax_terms(y, MU, torch.where(floored, torch.full_like(var, floor), var), float(eps))
            dv = torch.where(floored, torch.zeros_like(dv), dv)
            res.update(out=torch.stack([ell.sum(), torch.zeros((), dtype=torch.float64), dv.sum()]), dmu=dMU.T.contiguous(), dv=dv)
            if want_adjoints:
                res.update(g=(a.T @ dMU).T.contiguous(), G=(a * dv[:, None]).T @ a)
                T = dv[:, None] * T - dMU @ V / (2.0 * sf2)
        t_out[: N * M] = T.reshape(-1)
        return res

    def sgpmc_mc_tail(self, rows, V, N, kuu_linv, with_adjoints=False, result=None, vbar_out=None):
        self.calls["sgpmc_mc_tail"] += 1
        Cn, M = V.shape
        buf, out, info = result if result is not None else self.result_buffer()
        res = {"out": out, "info": info, "buf": buf}
        data = float(rows["out"][0])
        prior = -0.5 * float((V * V).sum()) - 0.5 * M * Cn * math.log(2.0 * math.pi)
        out.zero_()
        out[0], out[1], out[2] = data + prior, data, prior
        out[3], out[4] = 0.0, (float(rows["out"][2]) / N if N > 0 else 0.0)
        if with_adjoints:
            Li = kuu_linv
            g, G = rows["g"], rows["G"]
            S = 0.5 * (G + G.T)
            for c in range(Cn):
                P = torch.outer(V[c], g[c])
                lowP = torch.tril(P, -1) + 0.5 * torch.diag(torch.diagonal(P))
                S = S - 0.5 * (lowP + lowP.T)
            vbar = g - V
            if vbar_out is not None:
                vbar_out[: Cn * M].copy_(vbar.reshape(-1))
                vbar = vbar_out[: Cn * M].view(Cn, M)
            res.update(vbar=vbar, bbar=(Li.T @ V.T).T.contiguous(), Kuubar=Li.T @ S @ Li)
        return res
