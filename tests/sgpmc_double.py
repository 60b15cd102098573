"""CPU double of the engine for the SGPMC path: ``FactoredOracleEngine`` + ``sgpmc_tail`` and the zero-``LS`` predictive.

TEST INFRASTRUCTURE ONLY -- torch fp64 on the host, so that ``targets.SgpmcTarget``, ``hmc.sample_hmc`` and ``sgp_hmc`` run in a
container without a GPU.  ``sgpmc_tail`` restates include/sgp.h (sgp_sgpmc_from_whitened_stats) from the whitened statistics it is
handed; tests/test_sgpmc.py holds the target over this double to autograd of tests/sgpmc_reference.py."""
import math

import torch

from fake_engine import KID, FactoredOracleEngine
from oracle import vfe_oracle as O


class SgpmcOracleEngine(FactoredOracleEngine):
    def __init__(self):
        super().__init__()
        self.calls.update({"sgpmc_tail": 0, "svgp_predict": 0})

    COND_LIMIT = 1e13

    def kuu_factor(self, Kuu, info=None, trace_out=None):
        """... with the library's conditioning gate (include/sgp.h: sgp_set_cond_limit): a factor whose estimate
        max(max_j |L e_j|^2, |L^T 1|^2 / M) x max_i |e_i^T L^-1|^2 <= cond(K_uu) exceeds 1e13 is reported as not positive definite at
        that row of L^-1 -- LAPACK's factorization alone can pass an exactly singular K_uu on a rounding-sized pivot."""
        Li, info = super().kuu_factor(Kuu, info, trace_out)
        if int(info[0]) == 0:
            M = Kuu.shape[0]
            L = torch.linalg.solve_triangular(Li, torch.eye(M, dtype=torch.float64), upper=False)
            lam = max(float((L * L).sum(0).max()), float((L.sum(0) ** 2).sum()) / M)
            rows = (Li * Li).sum(1)
            if not lam * float(rows.max()) <= self.COND_LIMIT:
                info[0] = int(rows.argmax()) + 1
        return Li, info

    def sgpmc_tail(self, packed_whitened, v, s2, N, kuu_linv, with_adjoints=False, result=None, vbar_out=None):
        self.calls["sgpmc_tail"] += 1
        M = int(v.numel())
        W = packed_whitened[: M * M].reshape(M, M)
        W = 0.5 * (W + W.T)
        u = packed_whitened[M * M: M * M + M]
        yy, kappa = float(packed_whitened[M * M + M]), float(packed_whitened[M * M + M + 1])
        s2 = float(s2)
        buf, out, info = result if result is not None else self.result_buffer()
        res = {"out": out, "info": info, "buf": buf}
        Wv = W @ v
        Q = yy - 2.0 * float(v @ u) + float(v @ Wv) + kappa - float(torch.trace(W))
        data = -0.5 * N * math.log(2.0 * math.pi * s2) - Q / (2.0 * s2)
        prior = -0.5 * float(v @ v) - 0.5 * M * math.log(2.0 * math.pi)
        out.zero_()
        out[0], out[1], out[2] = data + prior, data, prior
        out[3], out[4] = -0.5 * N / s2 + Q / (2.0 * s2 * s2), -1.0 / (2.0 * s2)
        if with_adjoints:
            Li = kuu_linv[:M, :M] if kuu_linv.dim() == 2 else kuu_linv.view(-1)[: M * M].view(M, M)
            h = (u - Wv) / s2
            T = torch.outer(v, h)
            lowT = torch.tril(T, -1) + 0.5 * torch.diag(torch.diagonal(T))
            S = -W / (2.0 * s2) - 0.5 * (lowT + lowT.T)
            vbar = h - v
            if vbar_out is not None:
                vbar_out[:M].copy_(vbar)
                vbar = vbar_out
            res.update(vbar=vbar, Cw=torch.eye(M, dtype=torch.float64) - torch.outer(v, v), bbar=Li.T @ v / s2, Kuubar=Li.T @ S @ Li)
        return res

    def svgp_predict(self, Xs, Z, ls, sf2, m, LS, jitter=1e-6, kernel="rbf"):
        """The whitened SVGP predictive; with LS = 0 (a point mass at v = m) exactly mean = a^T v, var = k** - |a|^2, a = L^-1 k_u*."""
        if float(LS.abs().max()) != 0.0:
            return super().svgp_predict(Xs, Z, ls, sf2, m, LS, jitter, kernel)
        self.calls["svgp_predict"] += 1
        lst = self._ls(ls, Z.shape[1])
        K = O.kuu(Z, lst, float(sf2), float(jitter), KID[kernel])
        a = torch.linalg.solve_triangular(torch.linalg.cholesky(K), O.kern(Z, Xs, lst, float(sf2), KID[kernel]), upper=False)
        return a.T @ m, float(sf2) - (a * a).sum(0), torch.zeros(1, dtype=torch.int32)
