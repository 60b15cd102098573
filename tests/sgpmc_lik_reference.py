"""Long-double reference of SGPMC with a non-conjugate likelihood (include/sgp.h: sgp_sgpmc_lik_rows, sgp_sgpmc_lik_tail), of the
complete gradient behind them, and of the two new per-datum likelihoods for tests/svgp_reference.py.

TEST INFRASTRUCTURE ONLY -- numpy ``longdouble`` on the host, in the style of tests/svgp_reference.py, whose forward pass, kernel
adjoint, Gauss-Hermite rule and log Phi it imports.  With K = K_uu + J I, L = chol(K), A = L^-1 K_uf (M x N, column n is a_n):

    mu = A^T v     var = sf2 - colsum(A o A)  (raised to 2^-40 sf2, its derivative 0 there)     ell_n = E_{N(mu_n, var_n)} log p(y_n | f)
    rows:  out = [sum ell | sum d ell / d s2 | sum dv]     g = A dmu     G = (A diag(dv)) A^T     dmu, dv per datum
    tail:  F = sum ell - v.v / 2 - M/2 log 2 pi     vbar = g - v     bbar = L^-T v     Kuubar = L^-T (G - sym(low(v g^T))) L^-1

The complete gradient dF / d{v, ls, sf2, s2, Z} is formed IN ROW SPACE, as the SVGP reference forms its own (q(u) a point mass at v):

    Abar = v dmu^T - 2 A diag(dv)     Kufbar = L^-T Abar     Lbar = -tril(Kufbar A^T)     Kuubar' = sym(L^-T low(L^T Lbar) L^-1)
    g_sf2 = sum(Kufbar o k'_uf) + sum(Kuubar' o k'_uu) + sum dv,   g_ls, g_Z through dk'/dr2

-- that is, WITHOUT the two reuse arguments of the device code.  Those are restated beside it (the keys "reuse_*"): Kuubar from the
tail's formula, and the N-side adjoint as the factored pass 2 forms it, Kfubar = sf2 T_in (Cw / s2) L^-1 + y bbar^T with T_in =
diag(dv) T, y := dmu, bbar := L^-T v, Cw := -2 I, s2 := 1, kappabar := sum dv / N.  tests/test_sgpmc_lik_reference.py holds the two
routes to each other; ``mutate`` breaks the reuse route (or the likelihood) in one way so that a test can show the comparison failing.

``reference`` returns (ref, A): A is the CONDITION SCALE of each component -- the same sums with every factor replaced by its absolute
value, carried to first order through the quadrature and through exp() -- and the comparison is |got - ref| <= tol * A.
``dtype=np.float64`` runs the same closed form in float64 (``measure_e64``: the float64 level of a cell).
"""
import functools
import math

import numpy as np

import svgp_reference as SR
from pass2_reference import KID, LD, worst_ratio
from sgpmc_reference import low, sym
from svgp_reference import _f64, _forward, _kernel_bwd, gauss_hermite, log_ndtr  # noqa: F401

LIK = {"gaussian": 0, "bernoulli": 1, "bernoulli_logit": 2, "poisson": 3}
MUTATIONS = ("dv_second_derivative", "no_low", "no_kappabar", "drop_row", "unscaled_T", "no_lgamma")
ROWS_KEYS = ("out", "G", "g", "dmu", "dv")
TAIL_KEYS = ("F", "data", "prior", "vbar", "bbar", "Kuubar")
GRAD_KEYS = ("g_v", "g_ls", "g_sf2", "g_s2", "g_Z")
FLOOR_SCALE = 2.0 ** -40
# The scales are float64 sums of the quadrature's own terms: at a confident, correctly labelled datum (y f ~ +65 under the probit link)
# every term phi / Phi underflows float64 and the sum is 0, while the long-double value is 1e-939.  No float64 result can be held to a
# relative accuracy below the format's smallest normal number, so that number is part of every per-datum scale of the two quadratures.
TINY = float(np.finfo(np.float64).tiny)


def _lgamma1(y, F):
    """log Gamma(y + 1) for non-negative integer counts: the sum of logs in F (math.lgamma beyond 10^4)."""
    out = np.zeros(y.shape, F)
    for i, c in enumerate(np.asarray(y, dtype=np.float64)):
        c = int(round(c))
        out[i] = np.log(np.arange(2, c + 1).astype(F)).sum() if c <= 10000 else F(math.lgamma(c + 1.0))
    return out


def expected_log_lik(y, mu, v, a_mu, a_v, s2, lik, F, mutate=None):
    """svgp_reference._expected_log_lik for the four likelihood ids: ((ell, d ell/d mu, d ell/d v, d ell/d s2, zmin), scales)."""
    if lik == 0:
        return _EXPECTED_0_1(y, mu, v, a_mu, a_v, s2, lik, F)
    if lik == 1 and mutate != "dv_second_derivative":
        out, (a_ell, a_emu, a_ev, a_es2) = _EXPECTED_0_1(y, mu, v, a_mu, a_v, s2, lik, F)
        return out, (a_ell + TINY, a_emu + TINY, a_ev + TINY, a_es2)
    yabs = np.abs(_f64(y))
    if lik == 3:
        E = np.exp(mu + v / 2)
        lg = np.zeros_like(mu) if mutate == "no_lgamma" else _lgamma1(y, F)
        E6 = _f64(E) * (1 + a_mu + a_v / 2)          # |E| and what A_mu, A_v do to it to first order
        a_ell = yabs * a_mu + E6 + _f64(lg)
        return (y * mu - E - lg, y - E, -E / 2, np.zeros_like(mu), None), (a_ell, yabs + E6, E6 / 2, np.zeros_like(a_mu))
    x, w = gauss_hermite(F)
    sd = np.sqrt(v)
    z = y[:, None] * (mu[:, None] + sd[:, None] * x[None, :])
    if lik == 1:
        lp = log_ndtr(z, F)
        r = np.exp(-z * z / 2 - np.log(2 * np.arccos(F(-1))) / 2 - lp)
        curv = r * (z + r)                           # -(log Phi)''
    else:
        lp = -np.logaddexp(F(0), -z)                 # log sigmoid(z)
        r = np.exp(-np.logaddexp(F(0), z))           # sigmoid(-z) = (log sigmoid)'
        curv = r * (1 - r)
    ell = (lp * w).sum(1)
    wyr = w * y[:, None] * r
    e_mu = wyr.sum(1)
    e_v = (wyr * x).sum(1) / (2 * sd)
    if mutate == "dv_second_derivative":             # Price's theorem: d/dv E f = E f'' / 2 -- not the derivative of the quadrature sum
        e_v = -(w * curv).sum(1) / 2
    w6, x6, r6, sd6 = _f64(w), np.abs(_f64(x)), _f64(r), _f64(sd)
    rp = np.abs(_f64(curv))
    s_r, s_rx = (w6 * r6).sum(1), (w6 * r6 * x6).sum(1) / (2 * sd6)
    s_p, s_px, s_pxx = (w6 * rp).sum(1), (w6 * rp * x6).sum(1) / (2 * sd6), (w6 * rp * x6 * x6).sum(1) / (4 * sd6 * sd6)
    a_ell = (w6 * np.abs(_f64(lp))).sum(1) + s_r * a_mu + s_rx * a_v
    a_emu = s_r + s_p * a_mu + s_px * a_v
    a_ev = s_rx + s_px * a_mu + (s_pxx + s_rx / (2 * sd6 * sd6)) * a_v
    return (ell, e_mu, e_v, np.zeros_like(mu), float(z.min())), (a_ell + TINY, a_emu + TINY, a_ev + TINY, np.zeros_like(a_mu))


_EXPECTED_0_1 = SR._expected_log_lik


def svgp_reference_lik(*args, **kw):
    """``svgp_reference.reference`` with the per-datum functions of this file supplied (likelihood ids 2 and 3 as well)."""
    SR._expected_log_lik = expected_log_lik
    try:
        return SR.reference(*args, **kw)
    finally:
        SR._expected_log_lik = _EXPECTED_0_1


def _c(a, F):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return (a if a.dtype == LD else a.astype(np.float64)).astype(F)


def reference(X, y, Z, ls, sf2, s2, jitter, kernel, lik, v, dtype=LD, mutate=None, grads=True):
    """(ref, A) of every output of the two entry points (ROWS_KEYS, TAIL_KEYS, "s2bar", "kappabar", and ref["mu"], ref["var"],
    ref["floored"]), and with ``grads`` the complete gradient (GRAD_KEYS) in row space beside the reuse route ("reuse_" + GRAD_KEYS,
    "reuse_Kfubar", "row_Kfubar", "row_Kuubar", "S")."""
    assert mutate is None or mutate in MUTATIONS
    F = dtype
    kid = KID[kernel]
    lik = LIK.get(lik, lik)
    X, y, Z, ls, v = _c(X, F), _c(y, F).reshape(-1), _c(Z, F), _c(ls, F).reshape(-1), _c(v, F).reshape(-1)
    sf2, s2 = F(_c(sf2, F)), F(_c(s2, F))
    N, M = X.shape[0], Z.shape[0]
    f = _forward(X, Z, ls, sf2, v, np.zeros((M, M), F), jitter, kid, F)
    Am, Li, L, aA, aLi = f["A"], f["Li"], f["L"], f["aA"], f["aLi"]
    mu, var, a_mu, a_v = f["mu"], f["v"], f["a_mu"], f["a_v"]
    floor = sf2 * F(FLOOR_SCALE)
    floored = var < floor
    (ell, e_mu, e_v, e_s2, zmin), (a_ell, a_emu, a_ev, a_es2) = expected_log_lik(y, mu, np.where(floored, floor, var), a_mu, a_v, s2, lik, F,
                                                                                 mutate)
    e_v, a_ev = np.where(floored, F(0), e_v), np.where(floored, 0.0, a_ev)
    e_s2, a_es2 = e_s2 * np.ones(N, F), a_es2 * np.ones(N)
    if mutate == "drop_row":
        for t in (ell, e_mu, e_v, e_s2):
            t[N - 1] = 0
    av = np.abs(_f64(v))
    g, a_g = Am @ e_mu, aA @ a_emu
    G, a_G = (Am * e_v) @ Am.T, (aA * a_ev) @ aA.T
    LOG2PI = np.log(2 * np.arccos(F(-1)))
    data, prior = ell.sum(), -(v @ v) / 2 - F(M) / 2 * LOG2PI
    a_prior = float((v @ v) / 2 + F(M) / 2 * LOG2PI)
    chol_adj = np.zeros((M, M), F) if mutate == "no_low" else sym(low(np.outer(v, g)))
    Sp, a_Sp = G - chol_adj, a_G + sym(low(np.outer(av, a_g)))
    ref = {"out": np.array([data, e_s2.sum(), e_v.sum()]), "G": G, "g": g, "dmu": e_mu, "dv": e_v, "F": data + prior, "data": data, "prior": prior,
           "vbar": g - v, "bbar": Li.T @ v, "Kuubar": Li.T @ Sp @ Li, "s2bar": e_s2.sum(), "kappabar": e_v.sum() / max(N, 1),
           "mu": mu, "var": var, "floored": floored, "zmin": zmin}
    A = {"out": np.array([a_ell.sum(), a_es2.sum(), a_ev.sum()]), "G": a_G, "g": a_g, "dmu": a_emu, "dv": a_ev, "F": a_ell.sum() + a_prior,
         "data": a_ell.sum(), "prior": a_prior, "vbar": a_g + av, "bbar": aLi.T @ av, "Kuubar": aLi.T @ a_Sp @ aLi, "s2bar": a_es2.sum(),
         "kappabar": a_ev.sum() / max(N, 1)}
    if not grads:
        return ref, A
    # ---- row space (the SVGP reference's closed form with L_S = 0) ----
    Abar, a_Abar = np.outer(v, e_mu) - 2 * Am * e_v, np.outer(av, a_emu) + 2 * aA * a_ev
    Kufbar, a_Kufbar = Li.T @ Abar, aLi.T @ a_Abar
    Lbar, a_Lbar = -np.tril(Kufbar @ Am.T), np.tril(a_Kufbar @ aA.T)
    Kuubar_row = sym(Li.T @ low(L.T @ Lbar) @ Li)
    a_Kuubar = sym(aLi.T @ low(np.abs(_f64(L)).T @ a_Lbar) @ aLi)
    (s_uf, l_uf, z_uf), (as_uf, al_uf, az_uf) = _kernel_bwd(X, Z, ls, sf2, Kufbar.T, a_Kufbar.T, kid, kid, F, False)
    (s_uu, l_uu, z_uu), (as_uu, al_uu, az_uu) = _kernel_bwd(Z, Z, ls, sf2, Kuubar_row, a_Kuubar, kid, kid, F, False)
    ref.update(g_v=g - v, g_sf2=s_uf + s_uu + e_v.sum(), g_ls=l_uf + l_uu, g_Z=z_uf + 2 * z_uu, g_s2=e_s2.sum(),
               row_Kfubar=Kufbar.T, row_Kuubar=Kuubar_row)
    A.update(g_v=a_g + av, g_sf2=as_uf + as_uu + a_ev.sum(), g_ls=al_uf + al_uu, g_Z=az_uf + 2 * az_uu, g_s2=a_es2.sum(),
             row_Kfubar=a_Kufbar.T, row_Kuubar=a_Kuubar)
    # ---- the reuse route: the tail's Kuubar and the factored pass 2's own formula ----
    T = Am.T / sf2                                             # unit amplitude, N x M: what T_out holds after the product
    # G = -S^T S.  dv <= 0 as a sum (the weights are symmetric and (log p)' is monotone), but where every node is saturated it is rounding
    # noise of either sign around 0, 1e-20 here: the device sets a positive dv to 0 before it takes the root, and so does S.
    ref["S"] = np.sqrt(np.maximum(-e_v, 0))[:, None] * Am.T
    T_in = T if mutate == "unscaled_T" else e_v[:, None] * T
    Cw, s2_pass2 = -2 * np.eye(M, dtype=F), F(1)
    Kfubar = sf2 * (T_in @ (Cw / s2_pass2)) @ Li + np.outer(e_mu, ref["bbar"])
    (r_uf, rl_uf, rz_uf), _ = _kernel_bwd(X, Z, ls, sf2, Kfubar, a_Kufbar.T, kid, kid, F, False)
    (r_uu, rl_uu, rz_uu), _ = _kernel_bwd(Z, Z, ls, sf2, ref["Kuubar"], a_Kuubar, kid, kid, F, False)
    kappabar = F(0) if mutate == "no_kappabar" else ref["kappabar"]
    ref.update(reuse_Kfubar=Kfubar, reuse_g_v=ref["vbar"], reuse_g_sf2=r_uf + r_uu + kappabar * N, reuse_g_ls=rl_uf + rl_uu,
               reuse_g_Z=rz_uf + 2 * rz_uu, reuse_g_s2=ref["s2bar"])
    for k in GRAD_KEYS:
        A["reuse_" + k] = A[k]
    A["reuse_Kfubar"] = A["row_Kfubar"]
    return ref, A


# ---------------------------------------------------------------------------------------------------------------------------------
# the cells of tests/test_sgpmc_lik_gpu.py (and of the CPU tests that measure its tolerance)
# ---------------------------------------------------------------------------------------------------------------------------------
# (N, M, d): each the smallest shape reaching its branch -- see the GPU test's docstring
CELLS = [(1, 1, 1), (63, 5, 1), (255, 64, 2), (256, 64, 2), (257, 65, 3), (300, 129, 9), (200, 130, 32), (600, 300, 2), (65537, 5, 1)]
_ALL = ("gaussian", "bernoulli", "bernoulli_logit", "poisson")
# (kernel, likelihood, scale of v): rbf on every cell, the Matern kernels on two, every likelihood, v = 0 / N(0, 1) / 30 N(0, 1)
COMBOS = {
    (1, 1, 1): [("rbf", l, 1.0) for l in _ALL],
    (63, 5, 1): [("rbf", l, s) for l in _ALL for s in (0.0, 1.0, 30.0)] + [("matern32", "poisson", 1.0), ("matern52", "bernoulli_logit", 1.0)],
    (255, 64, 2): [("rbf", "poisson", 1.0), ("rbf", "bernoulli", 30.0)],
    (256, 64, 2): [("rbf", "bernoulli_logit", 1.0), ("rbf", "gaussian", 0.0)],
    (257, 65, 3): [("rbf", l, 1.0) for l in _ALL] + [("matern32", "bernoulli", 1.0), ("matern52", "poisson", 1.0)],
    (300, 129, 9): [("rbf", "poisson", 1.0), ("rbf", "bernoulli_logit", 30.0)],
    (200, 130, 32): [("rbf", "bernoulli", 1.0), ("rbf", "poisson", 0.0)],
    (600, 300, 2): [("rbf", "poisson", 1.0)],
    (65537, 5, 1): [("rbf", "poisson", 1.0), ("rbf", "bernoulli_logit", 1.0)],
}
S2 = 0.1   # the Gaussian likelihood's noise variance in every cell


@functools.lru_cache(maxsize=None)
def cell_inputs(N, M, d, lik, vscale):
    """Inputs of a cell (float64 numpy, read-only): X, Z, ls, sf2, jitter of ``svgp_reference.cell_inputs`` (the first min(3, M, N)
    rows of X are rows of Z; (63, 5, 1) is its ill-conditioned cell, lengthscale 3.5 spacings), labels / counts / targets drawn from
    its latent function, and v = vscale x standard normal."""
    base = SR.cell_inputs(N, M, d, "bernoulli" if lik in ("bernoulli", "bernoulli_logit") else "gaussian")
    rng = np.random.default_rng(7 + 1000003 * N + 1009 * M + d)
    X = base["X"]
    if lik == "poisson":
        fn = np.sin(1.3 * X[:, 0]) + 0.5 * np.cos(X[:, (1 % d)] + 0.3)
        y = rng.poisson(np.exp(fn)).astype(np.float64)
    else:
        y = np.array(base["y"])
    v = vscale * np.random.default_rng(11 + M).standard_normal(M)
    out = dict(X=X, y=y, Z=base["Z"], ls=base["ls"], sf2=base["sf2"], s2=S2 if lik == "gaussian" else 1.0, jitter=base["jitter"], v=v)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cell_reference(N, M, d, kernel, lik, vscale, dtype=LD, mutate=None, grads=True):
    """(ref, A) of a cell, cached: several tests share a cell."""
    inp = cell_inputs(N, M, d, lik, vscale)
    return reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["s2"], inp["jitter"], kernel, lik, inp["v"], dtype=dtype,
                     mutate=mutate, grads=grads)


ALL_KEYS = ROWS_KEYS + TAIL_KEYS + ("s2bar", "kappabar") + GRAD_KEYS


def worst(got, ref, A, keys=ALL_KEYS):
    """{key: worst |got - ref| / A over the key's components}"""
    return {k: worst_ratio(got[k], ref[k], A[k]) for k in keys if k in got}


def measure_e64(N, M, d, kernel, lik, vscale):
    """The float64 level of a cell: the worst |float64 closed form - long double| / A over every compared component."""
    ref, A = cell_reference(N, M, d, kernel, lik, vscale)
    r64, _ = cell_reference(N, M, d, kernel, lik, vscale, dtype=np.float64)
    return max(worst(r64, ref, A).values())
