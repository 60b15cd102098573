"""CPU double of the engine for SGPMC with a non-conjugate likelihood: ``SgpmcOracleEngine`` + ``sgpmc_lik_rows`` / ``sgpmc_lik_tail``.

TEST INFRASTRUCTURE ONLY -- torch fp64 on the host, so that ``targets.SgpmcTarget(likelihood=...)``, ``hmc.sample_hmc`` and ``sgp_hmc``
run in a container without a GPU.  The two methods restate include/sgp.h (sgp_sgpmc_lik_rows, sgp_sgpmc_lik_tail) with the likelihood
layer of csrc/sgp_lik.hpp: the 20-point Gauss-Hermite sums and THEIR derivatives, the variance floor 2^-40 sf2.  ``t_out`` is used as
the HIP engine uses it -- T = K'_fu L^-T on return of a value-only call, diag(dv) T with the adjoints -- and the factored pass 2 takes
whatever ``t_in`` it is handed: Kfubar = sf2 T_in (Cw / s2) L^-1 + y bbar^T, differentiated through the kernel by autograd."""
import math

import numpy as np
import torch

from fake_engine import KID
from oracle import vfe_oracle as O
from sgpmc_double import SgpmcOracleEngine

LIK = {"gaussian": 0, "bernoulli": 1, "bernoulli_probit": 1, "bernoulli_logit": 2, "poisson": 3}
_GX, _GW = np.polynomial.hermite.hermgauss(20)
GH_X = torch.as_tensor(_GX * math.sqrt(2.0))
GH_W = torch.as_tensor(_GW / math.sqrt(math.pi))


def lik_terms(lik, y, mu, var, s2):
    """(ell, dmu, dv, ds2) per datum, as csrc/sgp_lik.hpp forms them."""
    zero = torch.zeros_like(mu)
    if lik == 0:
        r = y - mu
        q = r * r + var
        return (-0.5 * math.log(2.0 * math.pi) - 0.5 * math.log(s2) - q / (2.0 * s2), r / s2, torch.full_like(mu, -0.5 / s2),
                -0.5 / s2 + q / (2.0 * s2 * s2))
    if lik == 3:
        E = torch.exp(mu + 0.5 * var)
        return y * mu - E - torch.lgamma(y + 1.0), y - E, -0.5 * E, zero
    sd = torch.sqrt(var)
    z = y[:, None] * (mu[:, None] + sd[:, None] * GH_X[None, :])
    if lik == 1:
        lp = torch.special.log_ndtr(z)
        r = torch.exp(-0.5 * z * z - 0.5 * math.log(2.0 * math.pi) - lp)
    else:
        lp = torch.nn.functional.logsigmoid(z)
        r = torch.sigmoid(-z)
    wyr = GH_W * y[:, None] * r
    return (lp * GH_W).sum(1), wyr.sum(1), (wyr * GH_X).sum(1) / (2.0 * sd), zero


class SgpmcLikOracleEngine(SgpmcOracleEngine):
    def __init__(self):
        super().__init__()
        self.calls.update({"sgpmc_lik_rows": 0, "sgpmc_lik_tail": 0})

    def sgpmc_lik_rows(self, X, y, Z, ls, sf2, s2, v, kuu_linv, t_out, kernel="rbf", likelihood="poisson", want_adjoints=False):
        self.calls["sgpmc_lik_rows"] += 1
        N, (M, d) = X.shape[0], Z.shape
        sf2 = float(sf2)
        T = O.kern(X, Z, self._ls(ls, d), 1.0, KID[kernel]) @ kuu_linv.T      # unit amplitude, N x M
        a = sf2 * T
        mu, var = a @ v, sf2 - (a * a).sum(1)
        floor = sf2 * 2.0 ** -40
        floored = var < floor
        ell, dmu, dv, ds2 = lik_terms(LIK[likelihood], y, mu, torch.where(floored, torch.full_like(var, floor), var), float(s2))
        dv = torch.where(floored | (dv > 0.0), torch.zeros_like(dv), dv)   # (a positive dv is rounding noise: 0, as on the device)
        res = {"out": torch.stack([ell.sum(), ds2.sum(), dv.sum()]), "dmu": dmu, "dv": dv}
        if want_adjoints:
            res.update(g=a.T @ dmu, G=(a * dv[:, None]).T @ a)
            T = dv[:, None] * T
        t_out[: N * M] = T.reshape(-1)
        return res

    def sgpmc_lik_tail(self, rows, v, N, kuu_linv, with_adjoints=False, result=None, vbar_out=None):
        self.calls["sgpmc_lik_tail"] += 1
        M = int(v.numel())
        buf, out, info = result if result is not None else self.result_buffer()
        res = {"out": out, "info": info, "buf": buf}
        data = float(rows["out"][0])
        prior = -0.5 * float(v @ v) - 0.5 * M * math.log(2.0 * math.pi)
        out.zero_()
        out[0], out[1], out[2] = data + prior, data, prior
        out[3], out[4] = float(rows["out"][1]), (float(rows["out"][2]) / N if N > 0 else 0.0)
        if with_adjoints:
            Li = kuu_linv
            g, G = rows["g"], rows["G"]
            P = torch.outer(v, g)
            lowP = torch.tril(P, -1) + 0.5 * torch.diag(torch.diagonal(P))
            S = 0.5 * (G + G.T) - 0.5 * (lowP + lowP.T)
            vbar = g - v
            if vbar_out is not None:
                vbar_out[:M].copy_(vbar)
                vbar = vbar_out
            res.update(vbar=vbar, bbar=Li.T @ v, Kuubar=Li.T @ S @ Li)
        return res

    def suffstats_bwd_factored(self, X, y, Z, ls, sf2, kuu_linv, Cw, s2, bbar, kappabar, kernel="rbf", want_gz=False, out=None,
                               t_in=None):
        """With ``t_in``: the library's own formula on whatever T it is handed (the parent class insists on T = K'_fu L^-T)."""
        if t_in is None:
            return super().suffstats_bwd_factored(X, y, Z, ls, sf2, kuu_linv, Cw, s2, bbar, kappabar, kernel, want_gz, out)
        self.calls["suffstats_bwd_factored"] += 1
        self.calls["t_handed_over"] += 1
        N, (M, d) = X.shape[0], Z.shape
        Kbar = float(sf2) * (t_in[: N * M].reshape(N, M) @ (Cw / float(s2))) @ kuu_linv + torch.outer(y, bbar)
        lst = self._ls(ls, d).clone().requires_grad_(True)
        sf2t = torch.tensor(float(sf2), dtype=torch.float64, requires_grad=True)
        Zt = Z.detach().clone().requires_grad_(True)
        loss = (O.kern(X, Zt, lst, sf2t, KID[kernel]) * Kbar).sum() + float(kappabar) * N * sf2t
        gl, gs, gz = torch.autograd.grad(loss, (lst, sf2t, Zt))
        g = torch.cat([gl, gs.reshape(1)] + ([gz.reshape(-1)] if want_gz else []))
        if out is not None:
            out[: g.numel()].copy_(g)
            return out
        return g
