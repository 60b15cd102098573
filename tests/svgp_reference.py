"""Long-double reference of the SVGP minibatch bound (csrc/sgp_svgp.hip), of its six gradients and of the latent predictive, with the
condition scale of every component.

TEST INFRASTRUCTURE ONLY -- numpy ``longdouble`` (x87 extended: eps 1.1e-19) on the host, no device code, no torch in the arithmetic
(the one exception: log Phi, see ``log_ndtr``).  It is the yardstick tests/test_svgp_kernel.py holds sgp_svgp_elbo, sgp_svgp_elbo_batch,
sgp_svgp_predict and sgp_svgp_predict_batch against, in the style of tests/pass2_reference.py.

Forward, with K = K_uu + J I, L = chol(K), L^-1 by substitution, Ls = tril(L_S):

    A = L^-1 K_ub     T = Ls^T A     mu = A^T m     v = sf2 - colsum(A o A) + colsum(T o T)
    ell_b = E_{N(mu_b, v_b)} log p(y_b | f):  Gaussian in closed form; Bernoulli-probit sum_i w_i log Phi(y_b (mu_b + sqrt(v_b) x_i)) on
            the 20-point rule of numpy.polynomial.hermite.hermgauss
    KL = (m.m + |Ls|_F^2 - M - 2 sum log diag Ls) / 2          bound per datum  F = mean_b ell_b - KL / N

Reverse, in closed form (nothing is differentiated through sqrt(r2), so r = 0 is no obstacle), mubar = (d ell / d mu) / B, vbar likewise:

    g_m  = A mubar - m / N                      g_LS = tril(2 (A diag(vbar) T^T)) - (Ls - diag(1 / diag Ls)) / N
    Abar = m mubar^T + 2 (Ls T - A) diag(vbar)  Kubbar = L^-T Abar            Lbar = -tril(Kubbar A^T)
    Kuubar = sym(L^-T low(L^T Lbar) L^-1)       (Cholesky adjoint, Murray 2016; low = lower triangle with the diagonal halved)
    g_sf2 = sum(Kubbar o k'_ub) + sum(Kuubar o k'_uu) + sum vbar,   g_ls and g_Z through dk'/dr2 as in pass2_reference.profile.

``reference`` returns (ref, A): two dicts with the same keys.  A is the CONDITION SCALE of the component: the same sums with every factor
replaced by its absolute value (|L^-1|, |Ls|, |m|, |y| ...); through the Bernoulli quadrature, which is no polynomial, the scale of
mu and v is carried on to first order (|d ell / d mu| A_mu + |d ell / d v| A_v, and the same for the two derivatives, with
|d(phi/Phi)/dz| = r (z + r)).  The scales are all-positive sums, so they are formed in float64.  The comparison is component-wise
|got - ref| <= tol * A  (``pass2_reference.worst_ratio``).

``dtype=np.float64`` runs the same closed form in float64 (what tests/test_svgp_reference.py measures the float64 error level with);
``mutate`` applies one deliberate defect (MUTATIONS) so that a test can show the comparison failing on it.
"""
import functools
import math

import numpy as np
import torch

from pass2_reference import KID, LD, worst_ratio
from sgpmc_reference import chol_ld, low, sym, tri_inv_ld

GH_POINTS = 20
MUTATIONS = ("drop_row", "drop_col", "h32_for_52", "kl_no_invdiag", "skip_r0")
KEYS = ("elbo", "ell_sum", "kl", "g_m", "g_LS", "g_Z", "g_ls", "g_sf2", "g_s2")


def profile(r2, kid, F):
    """(k', dk'/dr2) of the unit-amplitude profile in the dtype F (pass2_reference.profile with constants of that type)."""
    if kid == 0:
        k = np.exp(-r2 / 2)
        return k, -k / 2
    if kid == 1:
        a = np.sqrt(3 * r2)
        e = np.exp(-a)
        return (1 + a) * e, -(F(3) / 2) * e
    a = np.sqrt(5 * r2)
    e = np.exp(-a)
    return (1 + a + a * a / 3) * e, -(F(5) / 6) * (1 + a) * e


def log_ndtr(z, F=LD):
    """log Phi(z).  numpy has no long-double erfc: torch.special.log_ndtr in float64 (relative 1e-16 per term, and every term enters
    the bound with a weight <= 1), returned in F."""
    return torch.special.log_ndtr(torch.as_tensor(np.asarray(z, dtype=np.float64))).numpy().astype(F)


def gauss_hermite(F=LD, n=GH_POINTS):
    """Nodes / weights of  int f(x) N(x; 0, 1) dx  from numpy's physicists' rule."""
    x, w = np.polynomial.hermite.hermgauss(n)
    return x.astype(F) * np.sqrt(F(2)), w.astype(F) / np.sqrt(np.arccos(F(-1)))


def _f64(a):
    return np.asarray(a).astype(np.float64)


def _sqdist(Zs, Xs):
    D = Zs[:, None, :] - Xs[None, :, :]
    return (D * D).sum(-1)


def _kernel_bwd(rows, cols, ls, sf2, Kbar, Kabs, kid, hkid, F, skip_r0):
    """Gradient of sum(Kbar o sf2 k'(cols, rows)) with respect to ls, sf2 and the columns' inputs, and its scale from Kabs.
    rows: n x d, cols: M x d, Kbar / Kabs: n x M.  Returns ((s_sf2, g_ls, g_cols), (a_sf2, a_ls, a_cols))."""
    d = rows.shape[1]
    rs, cs = rows / ls, cols / ls
    D = [cs[None, :, j] - rs[:, j, None] for j in range(d)]          # D_j[n][m] = (z_mj - x_nj) / ls_j
    r2 = D[0] * D[0]
    for Dj in D[1:]:
        r2 = r2 + Dj * Dj
    kp = profile(r2, kid, F)[0]
    hp = profile(r2, hkid, F)[1]
    if skip_r0:
        keep = (r2 != 0).astype(F)
        Kbar, Kabs = Kbar * keep, Kabs * _f64(keep)
    E = Kbar * (sf2 * hp)
    Eabs = Kabs * _f64(sf2 * np.abs(hp))
    g_ls, a_ls = np.zeros(d, F), np.zeros(d)
    g_c, a_c = np.zeros(cols.shape, F), np.zeros(cols.shape)
    for j in range(d):
        g_ls[j] = -(2 / ls[j]) * np.einsum("nm,nm->", E * D[j], D[j])
        g_c[:, j] = (2 / ls[j]) * np.einsum("nm,nm->m", E, D[j])
        Dabs = _f64(np.abs(D[j]))
        a_ls[j] = float(2 / ls[j]) * np.einsum("nm,nm->", Eabs * Dabs, Dabs)
        a_c[:, j] = float(2 / ls[j]) * np.einsum("nm,nm->m", Eabs, Dabs)
    return (np.einsum("nm,nm->", Kbar, kp), g_ls, g_c), (np.einsum("nm,nm->", Kabs, _f64(kp)), a_ls, a_c)


def _expected_log_lik(y, mu, v, a_mu, a_v, s2, lik, F):
    """(ell, d ell/d mu, d ell/d v, d ell/d s2, zmin) per datum and the scales of the first four (float64)."""
    yabs = np.abs(_f64(y))
    if lik == 0:
        r = y - mu
        q = r * r + v
        ell = -np.log(2 * np.arccos(F(-1))) / 2 - np.log(s2) / 2 - q / (2 * s2)
        e_mu, e_v, e_s2 = r / s2, np.full_like(mu, -1 / (2 * s2)), -1 / (2 * s2) + q / (2 * s2 * s2)
        s = float(s2)
        a_r = yabs + a_mu
        a_q = a_r * a_r + a_v
        a_ell = math.log(2 * math.pi) / 2 + abs(math.log(s)) / 2 + a_q / (2 * s)
        return (ell, e_mu, e_v, e_s2, None), (a_ell, a_r / s, np.full_like(a_mu, 1 / (2 * s)), 1 / (2 * s) + a_q / (2 * s * s))
    x, w = gauss_hermite(F)
    sd = np.sqrt(v)
    z = y[:, None] * (mu[:, None] + sd[:, None] * x[None, :])
    lp = log_ndtr(z, F)
    r = np.exp(-z * z / 2 - np.log(2 * np.arccos(F(-1))) / 2 - lp)   # phi / Phi as exp(log phi - log Phi)
    ell = (lp * w).sum(1)
    wyr = w * y[:, None] * r
    e_mu = wyr.sum(1)
    e_v = (wyr * x).sum(1) / (2 * sd)
    # scales: the sums with absolute values plus what A_mu and A_v do to first order; |r'(z)| = r (z + r)
    w6, x6, r6, sd6 = _f64(w), np.abs(_f64(x)), _f64(r), _f64(sd)
    rp = r6 * np.abs(_f64(z) + r6)
    s_r, s_rx = (w6 * r6).sum(1), (w6 * r6 * x6).sum(1) / (2 * sd6)
    s_p, s_px, s_pxx = (w6 * rp).sum(1), (w6 * rp * x6).sum(1) / (2 * sd6), (w6 * rp * x6 * x6).sum(1) / (4 * sd6 * sd6)
    a_ell = (w6 * np.abs(_f64(lp))).sum(1) + s_r * a_mu + s_rx * a_v
    a_emu = s_r + s_p * a_mu + s_px * a_v
    a_ev = s_rx + s_px * a_mu + (s_pxx + s_rx / (2 * sd6 * sd6)) * a_v
    return (ell, e_mu, e_v, np.zeros_like(mu), float(z.min())), (a_ell, a_emu, a_ev, np.zeros_like(a_mu))


def _forward(X, Z, ls, sf2, m, Ls, jitter, kid, F, drop_col=False):
    M = Z.shape[0]
    K = sf2 * profile(_sqdist(Z / ls, Z / ls), kid, F)[0] + F(jitter) * np.eye(M, dtype=F)
    Kub = sf2 * profile(_sqdist(Z / ls, X / ls), kid, F)[0]          # M x B
    if drop_col:
        Kub[M - 1, :] = 0
    L = chol_ld(K, F)
    Li = tri_inv_ld(L, F)
    A = Li @ Kub
    T = Ls.T @ A
    mu = A.T @ m
    v = sf2 - (A * A).sum(0) + (T * T).sum(0)
    aLi, aLs = _f64(np.abs(Li)), _f64(np.abs(Ls))
    aA = aLi @ _f64(Kub)
    aT = aLs.T @ aA
    a_mu = aA.T @ np.abs(_f64(m))
    a_v = float(sf2) + (aA * aA).sum(0) + (aT * aT).sum(0)
    return dict(L=L, Li=Li, A=A, T=T, mu=mu, v=v, aLi=aLi, aLs=aLs, aA=aA, aT=aT, a_mu=a_mu, a_v=a_v)


def _prep(X, y, Z, ls, sf2, s2, m, LS, F):
    """Inputs in the dtype F; a long-double array or scalar is taken as it is (the central differences of the tests move inputs by
    less than a float64 resolves), everything else goes through float64."""
    def c(a):
        if hasattr(a, "detach"):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        return (a if a.dtype == LD else a.astype(np.float64)).astype(F)
    return c(X), (None if y is None else c(y).reshape(-1)), c(Z), c(ls).reshape(-1), F(c(sf2)), F(c(s2)), c(m).reshape(-1), np.tril(c(LS))


def reference(X, y, Z, ls, sf2, s2, m, LS, N_total, jitter, kernel, lik, dtype=LD, mutate=None, grads=True):
    """(ref, A) of sgp_svgp_elbo: KEYS (and ref["mu"], ref["v"], ref["zmin"]: the smallest Bernoulli argument y (mu + sqrt(v) x_i))."""
    assert mutate is None or mutate in MUTATIONS
    F = dtype
    kid = KID[kernel]
    X, y, Z, ls, sf2, s2, m, Ls = _prep(X, y, Z, ls, sf2, s2, m, LS, F)
    B, M, N = X.shape[0], Z.shape[0], F(N_total)
    f = _forward(X, Z, ls, sf2, m, Ls, jitter, kid, F, drop_col=(mutate == "drop_col"))
    (ell, e_mu, e_v, e_s2, zmin), (a_ell, a_emu, a_ev, a_es2) = _expected_log_lik(y, f["mu"], f["v"], f["a_mu"], f["a_v"], s2, lik, F)
    if mutate == "drop_row":
        for t in (ell, e_mu, e_v, e_s2):
            t[B - 1] = 0
    dg = np.diagonal(Ls)
    kl = ((m * m).sum() + (Ls * Ls).sum() - M - 2 * np.log(dg).sum()) / 2
    a_kl = float((m * m).sum() + (Ls * Ls).sum() + M + 2 * np.abs(np.log(dg)).sum()) / 2
    ref = {"elbo": ell.sum() / B - kl / N, "ell_sum": ell.sum(), "kl": kl, "mu": f["mu"], "v": f["v"], "zmin": zmin}
    A = {"elbo": a_ell.sum() / B + a_kl / float(N), "ell_sum": a_ell.sum(), "kl": a_kl, "mu": f["a_mu"], "v": f["a_v"]}
    if not grads:
        return ref, A
    Am, T, Li, L = f["A"], f["T"], f["Li"], f["L"]
    aA, aT, aLi, aLs = f["aA"], f["aT"], f["aLi"], f["aLs"]
    mub, vb = e_mu / B, e_v / B
    a_mub, a_vb = a_emu / B, a_ev / B
    am = np.abs(_f64(m))
    ref["g_m"], A["g_m"] = Am @ mub - m / N, aA @ a_mub + am / float(N)
    G, aG = (Am * vb) @ T.T, (aA * a_vb) @ aT.T
    inv_dg = np.zeros_like(dg) if mutate == "kl_no_invdiag" else 1 / dg
    ref["g_LS"] = np.tril(2 * G) - (Ls - np.diag(inv_dg)) / N
    A["g_LS"] = np.tril(2 * aG) + (aLs + np.diag(1 / np.abs(_f64(dg)))) / float(N)
    Abar = np.outer(m, mub) + 2 * (Ls @ T - Am) * vb
    a_Abar = np.outer(am, a_mub) + 2 * (aLs @ aT + aA) * a_vb
    Kubbar, a_Kubbar = Li.T @ Abar, aLi.T @ a_Abar
    Lbar, a_Lbar = -np.tril(Kubbar @ Am.T), np.tril(a_Kubbar @ aA.T)
    Kuubar = sym(Li.T @ low(L.T @ Lbar) @ Li)
    a_Kuubar = sym(aLi.T @ low(np.abs(_f64(L)).T @ a_Lbar) @ aLi)
    hkid = 1 if (mutate == "h32_for_52" and kid == 2) else kid
    skip = mutate == "skip_r0"
    (s_ub, l_ub, z_ub), (as_ub, al_ub, az_ub) = _kernel_bwd(X, Z, ls, sf2, Kubbar.T, a_Kubbar.T, kid, hkid, F, skip)
    (s_uu, l_uu, z_uu), (as_uu, al_uu, az_uu) = _kernel_bwd(Z, Z, ls, sf2, Kuubar, a_Kuubar, kid, hkid, F, skip)
    ref["g_sf2"], A["g_sf2"] = s_ub + s_uu + vb.sum(), as_ub + as_uu + a_vb.sum()
    ref["g_ls"], A["g_ls"] = l_ub + l_uu, al_ub + al_uu
    ref["g_Z"], A["g_Z"] = z_ub + 2 * z_uu, az_ub + 2 * az_uu          # z_m is a row and a column of the symmetric K_uu
    ref["g_s2"], A["g_s2"] = e_s2.sum() / B, float(np.sum(a_es2)) / B
    return ref, A


def predict_reference(Xs, Z, ls, sf2, m, LS, jitter, kernel, dtype=LD):
    """((mu, v), (A_mu, A_v)) of the latent predictive at the rows of Xs (sgp_svgp_predict, sgp_svgp_predict_batch)."""
    F = dtype
    Xs, _, Z, ls, sf2, _, m, Ls = _prep(Xs, None, Z, ls, sf2, 1.0, m, LS, F)
    f = _forward(Xs, Z, ls, sf2, m, Ls, jitter, KID[kernel], F)
    return (f["mu"], f["v"]), (f["a_mu"], f["a_v"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the cells: inputs of tests/test_svgp_kernel.py and of the CPU tests that measure its tolerance
# ---------------------------------------------------------------------------------------------------------------------------------
CELLS = [(1, 1, 1), (63, 5, 1), (64, 64, 2), (65, 65, 3), (257, 128, 8), (300, 129, 9), (200, 130, 32), (1400, 300, 2), (16385, 5, 1)]
# The one deliberately ill-conditioned cell: lengthscale 3.5 spacings, cond(K_uu + J I) = 3.8e5 under rbf (the older fixtures: ~1e6 at
# M = 256).  It is the smallest-M cell with B > 1 because the scale A grows with sum_m |L^-1| and, under Bernoulli, once more through
# A_v: at 4.1 spacings (cond 1.2e6) the wrong-h mutation of tests/test_svgp_reference.py stands only 50x above the tolerance under
# matern52-bernoulli, at 3.5 it stands 300x above, and the detection condition asks for 100x.
ILL_CELL = (63, 5, 1)
ILL_LS = (3.5, 3.5)
JITTER = 1e-6


def combos(cell):
    """(kernel, likelihood) pairs run on a cell: the full cross up to M = 65, rbf-bernoulli and matern52-gaussian beyond."""
    if cell[1] <= 65:
        return [(k, l) for k in ("rbf", "matern32", "matern52") for l in ("gaussian", "bernoulli")]
    return [("rbf", "bernoulli"), ("matern52", "gaussian")]


@functools.lru_cache(maxsize=None)
def cell_inputs(B, M, d, lik, distinct=False):
    """Inputs of a cell (float64 numpy, read-only).  Z sits on a unit grid over the first g = min(d, ceil(log2 M)) dimensions (the
    first M points in lexicographic order, ceil(M^(1/g)) per axis), every coordinate jittered by U(-0.15, 0.15); the lengthscales are
    0.55 .. 0.7 of the spacing on the grid axes (3.5 on ILL_CELL), 1.5 .. 2 on the others: cond(K_uu) stays below ~1e2 under rbf
    (tests/test_svgp_reference.py asserts the bound 1e4).  X: uniform over the grid's box, the first min(3, M, B) rows equal to rows
    of Z (r = 0) unless ``distinct``."""
    rng = np.random.default_rng(1000003 * B + 1009 * M + d)
    g = min(d, max(1, math.ceil(math.log2(M)))) if M > 1 else 1
    n = 1
    while n ** g < M:
        n += 1
    idx = np.stack(np.unravel_index(np.arange(M), (n,) * g), 1).astype(np.float64)
    Z = np.zeros((M, d))
    Z[:, :g] = idx
    Z += rng.uniform(-0.15, 0.15, (M, d))
    hi = Z[:, :g].max(0) + 0.5
    X = np.concatenate([rng.uniform(0, 1, (B, g)) * (hi + 0.5) - 0.5, rng.uniform(-0.3, 0.3, (B, d - g))], 1)
    if not distinct:
        k = min(3, M, B)
        X[:k] = Z[rng.permutation(M)[:k]]
    ill = (B, M, d) == ILL_CELL
    ls = np.concatenate([rng.uniform(*ILL_LS, g) if ill else rng.uniform(0.55, 0.7, g), rng.uniform(1.5, 2.0, d - g)])
    fn = np.sin(1.3 * X[:, 0]) + 0.5 * np.cos(X[:, (1 % d)] + 0.3)
    noise = rng.standard_normal(B)
    y = np.where(fn + 0.3 * noise > 0, 1.0, -1.0) if lik == "bernoulli" else fn + 0.2 * noise
    m = 0.3 * rng.standard_normal(M)
    LS = np.tril(0.1 * rng.standard_normal((M, M))) + np.eye(M)
    out = dict(X=X, y=y, Z=Z, ls=ls, sf2=1.3, s2=0.1 if lik == "gaussian" else 1.0, m=m, LS=LS, N_total=10 * B, jitter=JITTER)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


TAIL_CELL = (64, 5, 1)


@functools.lru_cache(maxsize=None)
def tail_inputs():
    """The Bernoulli tail cell (64, 5, 1): q(u) has the mean L m ~ +30 everywhere, sqrt(v) ~ 1.26, and three labels are -1 against it:
    their outer Gauss-Hermite node reaches z = -(30 + 1.26 * 7.62) < -39.1, beyond any binary64 erfc."""
    B, M, d = TAIL_CELL
    inp = dict(cell_inputs(B, M, d, "bernoulli"))
    Zs = inp["Z"] / inp["ls"]
    sf2 = 1.6
    K = sf2 * np.exp(-_sqdist(Zs, Zs) / 2) + JITTER * np.eye(M)
    m = np.linalg.solve(np.linalg.cholesky(K), np.full(M, 30.0))
    y = np.ones(B)
    y[[0, 17, 40]] = -1.0          # row 0 is a row of Z
    LS = np.array(inp["LS"])
    inp.update(sf2=sf2, m=m, y=y, LS=LS)
    for a in (m, y, LS):
        a.setflags(write=False)
    return inp


def theta_samples(inp, S):
    """S hyper-parameter samples around a cell's own (sample 0 is the cell's): ls S x d, sf2 S, s2 S."""
    rng = np.random.default_rng(77 + S)
    f = np.exp(0.1 * rng.standard_normal((S, inp["ls"].size + 2)))
    f[0] = 1.0
    return inp["ls"][None, :] * f[:, 2:], inp["sf2"] * f[:, 0], inp["s2"] * f[:, 1]


@functools.lru_cache(maxsize=None)
def cell_reference(B, M, d, kernel, lik, dtype=LD, mutate=None, tail=False, S=0, k=0, grads=True):
    """(ref, A) of a cell, cached: several tests share a cell.  ``S``, ``k``: sample k of ``theta_samples(inp, S)`` instead."""
    inp = tail_inputs() if tail else cell_inputs(B, M, d, lik)
    ls, sf2, s2 = inp["ls"], inp["sf2"], inp["s2"]
    if S:
        lss, sf2s, s2s = theta_samples(inp, S)
        ls, sf2, s2 = lss[k], sf2s[k], s2s[k]
    return reference(inp["X"], inp["y"], inp["Z"], ls, sf2, s2, inp["m"], inp["LS"], inp["N_total"], inp["jitter"], kernel,
                     1 if lik == "bernoulli" else 0, dtype=dtype, mutate=mutate, grads=grads)


def worst(got, ref, A, keys=KEYS):
    """{key: worst |got - ref| / A over the key's components}; ``got`` maps the keys to arrays / tensors / numbers."""
    return {k: worst_ratio(got[k], ref[k], A[k]) for k in keys if k in got}
