"""CPU double of the engine for SGPMC with a composite kernel, a white-noise term and a mean function: ``SgpmcLikOracleEngine`` +
``sgpmc_comp_rows`` / ``sgpmc_comp_bwd`` and the composite branch of ``kuu`` / ``kuu_bwd``.

TEST INFRASTRUCTURE ONLY -- torch fp64 on the host over ``oracle.composite_oracle``, so that ``composite.CompositeSgpmcTarget``,
``hmc.sample_hmc`` and the model functions of ``sgp_hmc`` run in a container without a GPU.  The two methods restate include/sgp.h
(sgp_sgpmc_comp_rows, sgp_sgpmc_comp_bwd): T = K_fu L^-T with the full amplitude, k_nn = kdiag + white, the floor 2^-40 k_nn.  ``t_out``
is used as the HIP engine uses it (T on return of a value-only call, diag(dv) T with the adjoints), in this double's packed N x M layout;
the reverse call differentiates sum(Kfubar o k(X, Z)) through the oracle's kernel by autograd."""
import numpy as np
import torch

from oracle import composite_oracle as CO
from sgpmc_lik_double import LIK, SgpmcLikOracleEngine, lik_terms


def _blk(block):
    return torch.as_tensor(np.asarray([float(t) for t in block], dtype=np.float64))


def _block_grad(rows, cols, block, Kbar):
    """d sum(Kbar o k(rows, cols)) / d block at the slots that carry a parameter (zero elsewhere)."""
    st = np.asarray([float(t) for t in block], dtype=np.float64)
    with torch.enable_grad():
        b = _blk(block).clone().requires_grad_(True)
        (CO.composite_k(rows, cols, b, st) * Kbar).sum().backward()
    g = torch.zeros(CO.COMP_LEN, dtype=torch.float64)
    for i in CO.grad_slots(st):
        g[i] = b.grad[i]
    return g


class SgpmcCompOracleEngine(SgpmcLikOracleEngine):
    def __init__(self):
        super().__init__()
        self.calls.update({"sgpmc_comp_rows": 0, "sgpmc_comp_bwd": 0})

    def kuu(self, Z, ls, sf2, jitter, kernel="rbf"):
        if kernel != "composite":
            return super().kuu(Z, ls, sf2, jitter, kernel)
        return CO.composite_k(Z, Z, _blk(ls)) + float(jitter) * torch.eye(Z.shape[0], dtype=torch.float64)

    def kuu_bwd(self, Z, ls, sf2, Kuubar, grads, kernel="rbf", want_gz=False):
        if kernel != "composite":
            return super().kuu_bwd(Z, ls, sf2, Kuubar, grads, kernel, want_gz)
        self.calls["kuu_bwd"] += 1
        grads[: CO.COMP_LEN] += _block_grad(Z, Z, ls, Kuubar)
        return grads

    def sgpmc_comp_rows(self, X, y, Z, block, white, s2, v, kuu_linv, t_out, likelihood="gaussian", mean=None, want_adjoints=False,
                        want_moments=False):
        self.calls["sgpmc_comp_rows"] += 1
        N, M = X.shape[0], Z.shape[0]
        a = CO.composite_k(X, Z, _blk(block)) @ kuu_linv.T                    # rows a_n^T = (L^-1 k(Z, x_n))^T, N x M
        knn = CO.kdiag(block) + float(white)
        mu, var = a @ v + (mean if mean is not None else 0.0), knn - (a * a).sum(1)
        if y is None:
            t_out[: N * M] = a.reshape(-1)
            z = torch.zeros(N, dtype=torch.float64)
            return {"out": torch.zeros(3, dtype=torch.float64), "dmu": z, "dv": z.clone(), "mu": mu, "var": var}
        floor = knn * 2.0 ** -40
        floored = var < floor
        ell, dmu, dv, ds2 = lik_terms(LIK[likelihood], y, mu, torch.where(floored, torch.full_like(var, floor), var), float(s2))
        dv = torch.where(floored | (dv > 0.0), torch.zeros_like(dv), dv)
        res = {"out": torch.stack([ell.sum(), ds2.sum(), dv.sum()]), "dmu": dmu, "dv": dv}
        if want_moments:
            res.update(mu=mu, var=var)
        if want_adjoints:
            res.update(g=a.T @ dmu, G=(a * dv[:, None]).T @ a)
            a = dv[:, None] * a
        t_out[: N * M] = a.reshape(-1)
        return res

    def sgpmc_comp_bwd(self, X, dmu, Z, block, t_in, kuu_linv, bbar, out=None):
        self.calls["sgpmc_comp_bwd"] += 1
        N, M = X.shape[0], Z.shape[0]
        Kbar = -2.0 * t_in[: N * M].reshape(N, M) @ kuu_linv + torch.outer(dmu, bbar)
        g = _block_grad(X, Z, block, Kbar)
        if out is None:
            out = torch.zeros(CO.COMP_LEN + 1, dtype=torch.float64)
        out[: CO.COMP_LEN] = g
        return out
