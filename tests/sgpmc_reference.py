"""Reference of the SGPMC density (include/sgp.h: sgp_sgpmc_from_whitened_stats) and of its adjoints.

TEST INFRASTRUCTURE ONLY.  Two restatements, neither of which goes through the library's whitened matrix W:

* ``reference`` -- numpy ``longdouble`` (x87 extended: eps 1.1e-19) from the EXPLICIT K = K_uu + jitter I, Phi = K_uf K_fu and b = K_uf y:
  L = chol(K) and L^-1 by substitution in long double, t = L^-T v, and then

      v.u = t.b        v^T W v = t^T Phi t        tr W = sum((L^-1 Phi) o L^-1)        h = L^-1 (b - Phi t) / s2

  so  F = -N/2 log(2 pi s2) - Q / (2 s2) - v.v / 2 - M/2 log(2 pi),  Q = yy - 2 v.u + v^T W v + kappa - tr W,  and the adjoints
  vbar = h - v, Cw = I - v v^T, bbar = t / s2, kappabar = -1 / (2 s2), s2bar = -N / (2 s2) + Q / (2 s2^2),
  Kuubar = L^-T S' L^-1 with S' = -(L^-1 Phi L^-T) / (2 s2) - sym(low(v h^T)).
  It returns (ref, A): two dicts with the same keys.  A is the CONDITION SCALE of the component, the same sum with every factor
  replaced by its absolute value (|L^-1|, |Phi|, |b|, |v|), in the style of tests/pass2_reference.py; the comparison is
  |got - ref| <= TAU A  (``pass2_reference.assert_close``).
  ``low_mode``: "ok" (the density's adjoint), "dropped" (without the Cholesky-adjoint term) or "transposed" (the term applied as
  upper triangle) -- the two wrong forms exist so that a test can show the comparison failing on them.

* ``density_torch`` / ``logp_torch`` -- torch fp64 in GPflow's own op order (A = L^-1 K_uf; mean of the conditional A^T v, its
  variance k_nn - |A_n|^2), differentiable: what autograd is asked for dF/dv, dF/dtheta, dF/dZ.  ``logp_torch`` adds the
  transforms, the Gamma(2, 1) priors and the log sigmoid(x) terms of ``targets.SgpmcTarget``.
"""
import math

import numpy as np
import torch

from oracle import vfe_oracle as O
from pass2_reference import LD, _ld, _ls, profile

LOG2PI = np.log(2 * np.arccos(LD(-1)))  # log(2 pi) in long double
NOISE_FLOOR = 1e-6


def chol_ld(K, dtype=LD):
    """Lower Cholesky factor in long double (numpy.linalg has no longdouble kernels): row by row.  (``dtype``: the same loop in float64.)"""
    M = K.shape[0]
    L = np.zeros((M, M), dtype)
    for i in range(M):
        for j in range(i):
            L[i, j] = (K[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
        d = K[i, i] - L[i, :i] @ L[i, :i]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite at pivot %d" % (i + 1))
        L[i, i] = np.sqrt(d)
    return L


def tri_inv_ld(L, dtype=LD):
    """L^-1 by forward substitution in long double."""
    M = L.shape[0]
    Li = np.zeros((M, M), dtype)
    for i in range(M):
        Li[i, i] = 1 / L[i, i]
        if i:
            Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
    return Li


def kernel_blocks(X, y, Z, ls, sf2, jitter, kernel_id):
    """(K, Phi, b, yy, kappa) in long double: the explicit matrices the reference starts from."""
    X, y, Z = _ld(X), _ld(y).reshape(-1), _ld(Z)
    ls = _ls(ls, X.shape[1])
    sf2 = LD(float(sf2))
    Du = Z[:, None, :] / ls - (Z / ls)[None, :, :]
    K = sf2 * profile((Du * Du).sum(-1), kernel_id)[0] + LD(float(jitter)) * np.eye(Z.shape[0], dtype=LD)
    Df = Z[:, None, :] / ls - (X / ls)[None, :, :]
    Kuf = sf2 * profile((Df * Df).sum(-1), kernel_id)[0]
    return K, Kuf @ Kuf.T, Kuf @ y, y @ y, sf2 * X.shape[0]


def low(A):
    """lower triangle with the diagonal halved"""
    return np.tril(A, -1) + np.diag(np.diag(A)) / 2


def sym(A):
    return (A + A.T) / 2


def reference(K, Phi, b, yy, kappa, v, s2, N, low_mode="ok"):
    """(ref, A) of every output of the SGPMC tail, plus the whitened inputs it would be handed: ref["W"], ref["u"], ref["Linv"]."""
    K, Phi, b, v = (np.asarray(a, LD) for a in (K, Phi, b, v))
    yy, kappa, s2 = LD(yy), LD(kappa), LD(float(s2))
    M = K.shape[0]
    Li = tri_inv_ld(chol_ld(K))
    aLi, aPhi, ab, av = np.abs(Li), np.abs(Phi), np.abs(b), np.abs(v)
    t, at = Li.T @ v, aLi.T @ av
    vu, a_vu = t @ b, at @ ab
    vWv, a_vWv = t @ Phi @ t, at @ aPhi @ at
    trW, a_trW = ((Li @ Phi) * Li).sum(), ((aLi @ aPhi) * aLi).sum()
    Q, a_Q = yy - 2 * vu + vWv + kappa - trW, abs(yy) + 2 * a_vu + a_vWv + abs(kappa) + a_trW
    lead = LD(N) / 2 * (LOG2PI + np.log(s2))
    data, a_data = -lead - Q / (2 * s2), abs(lead) + a_Q / (2 * s2)
    prior = -(v @ v) / 2 - LD(M) / 2 * LOG2PI
    a_prior = (v @ v) / 2 + LD(M) / 2 * LOG2PI
    h, a_h = Li @ (b - Phi @ t) / s2, aLi @ (ab + aPhi @ at) / s2
    W, a_W = Li @ Phi @ Li.T, aLi @ aPhi @ aLi.T
    T, a_T = np.outer(v, h), np.outer(av, a_h)
    chol_adj = {"ok": sym(low(T)), "dropped": np.zeros_like(T), "transposed": sym(low(T.T))}[low_mode]
    S, a_S = -W / (2 * s2) - chol_adj, a_W / (2 * s2) + sym(low(a_T))
    ref = {"F": data + prior, "data": data, "prior": prior, "s2bar": -LD(N) / (2 * s2) + Q / (2 * s2 * s2), "kappabar": -1 / (2 * s2),
           "vbar": h - v, "Cw": np.eye(M, dtype=LD) - np.outer(v, v), "bbar": t / s2, "Kuubar": Li.T @ S @ Li,
           "W": W, "u": Li @ b, "Linv": Li, "h": h}
    A = {"F": a_data + a_prior, "data": a_data, "prior": a_prior, "s2bar": LD(N) / (2 * s2) + a_Q / (2 * s2 * s2), "kappabar": 1 / (2 * s2),
         "vbar": a_h + av, "Cw": np.eye(M, dtype=LD) + np.outer(av, av), "bbar": at / s2, "Kuubar": aLi.T @ a_S @ aLi}
    return ref, A


def reference_at(X, y, Z, ls, sf2, s2, jitter, kernel_id, v, low_mode="ok"):
    K, Phi, b, yy, kappa = kernel_blocks(X, y, Z, ls, sf2, jitter, kernel_id)
    return reference(K, Phi, b, yy, kappa, v, s2, np.asarray(X).shape[0], low_mode)


# ---------------------------------------------------------------------------------------------
# torch fp64, GPflow's op order, differentiable
# ---------------------------------------------------------------------------------------------
def density_torch(v, X, y, Z, ls, sf2, s2, jitter, kernel_id=0):
    """F(v, theta): sum_n E_{p(f_n | v)} log N(y_n | f_n, s2) + log N(v | 0, I) with p(f_n | v) = N(A_n^T v, k_nn - |A_n|^2)."""
    T = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))
    v, X, y, Z, ls, sf2, s2 = T(v), T(X), T(y).reshape(-1), T(Z), T(ls), T(sf2), T(s2)
    M, N = Z.shape[0], X.shape[0]
    K = O.kernel_from_r2(O.sqdist(Z, Z, ls), sf2, kernel_id) + float(jitter) * torch.eye(M, dtype=torch.float64)
    Kuf = O.kernel_from_r2(O.sqdist(Z, X, ls), sf2, kernel_id)
    L = torch.linalg.cholesky(K)
    A = torch.linalg.solve_triangular(L, Kuf, upper=False)
    mean = A.T @ v
    var = sf2 - (A * A).sum(0)
    data = -0.5 * N * torch.log(2.0 * math.pi * s2) - (((y - mean) ** 2).sum() + var.sum()) / (2.0 * s2)
    return data - 0.5 * (v @ v) - 0.5 * M * math.log(2.0 * math.pi)


def logp_torch(q, X, y, Z, jitter, kernel_id=0):
    """``SgpmcTarget.logp`` restated: q = [x_var | x_ls (d) | x_noise | v]; softplus transforms, the 1e-6 noise floor, Gamma(2, 1)
    at the constrained values and log sigmoid(x) for each transform."""
    d = Z.shape[1]
    sp = torch.nn.functional.softplus
    sf2, ls, s2 = sp(q[0]), sp(q[1:1 + d]), NOISE_FLOOR + sp(q[1 + d])
    F = density_torch(q[2 + d:], X, y, Z, ls, sf2, s2, jitter, kernel_id)
    cons = torch.cat([sf2.reshape(1), ls, s2.reshape(1)])
    return F + (torch.log(cons) - cons).sum() + torch.nn.functional.logsigmoid(q[:2 + d]).sum()
