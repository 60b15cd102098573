"""Long-double reference of SGPMC with the multi-class robust-max likelihood (include/sgp.h: sgp_sgpmc_mc_rows, sgp_sgpmc_mc_tail)
and of the complete gradient behind them.

TEST INFRASTRUCTURE ONLY -- numpy ``longdouble`` on the host, in the style of tests/sgpmc_lik_reference.py, whose forward pass, kernel
adjoint, Gauss-Hermite rule and log Phi it shares.  With K = K_uu + J I, L = chol(K), A = L^-1 K_uf (M x N, column n is a_n), C latent
functions with whitened inducing values V (C x M, class-major) and labels y_n in {0 .. C-1}:

    MU = A^T V^T (N x C)     var = sf2 - colsum(A o A)  (raised to 2^-40 sf2, its derivative 0 there)
    delta_nc = (mu_{n,y_n} - mu_nc) / sqrt var_n     p_n = sum_i w_i prod_{c != y_n} Phi(x_i + delta_nc)
    ell_n = p_n log(1 - eps) + (1 - p_n) log(eps / (C - 1))
    rows:  out = [sum ell | 0 | sum dv]     g_c = A dmu_c     G = (A diag(dv)) A^T     dmu (C x N), dv (N)
    tail:  F = sum ell - sum_c v_c.v_c / 2 - M C / 2 log 2 pi     vbar = g - V     bbar_c = L^-T v_c
           Kuubar = L^-T (G - sum_c sym(low(v_c g_c^T))) L^-1

dmu, dv are the derivatives of the quadrature sum.  dv has both signs.  The complete gradient dF / d{V, ls, sf2, Z} is formed IN ROW
SPACE (Abar = sum_c v_c dmu_c^T - 2 A diag(dv), as tests/sgpmc_lik_reference.py), without the reuse arguments of the device code; those
are restated beside it (the keys "reuse_*"): Kuubar from the tail's formula and the N-side adjoint as ONE factored pass 2 forms it from
the folded T_in = diag(dv) T - DMU V^T / (2 sf2) with Cw = -2 I, s2 = 1, y = 0, bbar = 0.  ``mutate`` breaks one thing so that a test
can show the comparison failing.

``reference`` returns (ref, A): A is the component-wise CONDITION SCALE -- the same sums with every factor replaced by its absolute
value, carried to first order through delta, the quadrature and exp().  The scale of the folded N-side adjoint is |T_in| |L^-1| with
|T_in| = |dv| |T| + |DMU| |V|^T / (2 sf2): the product V^T L^-1 is formed inside the N-side product there, so its scale is the
row-space one, |L^-T| (|V|^T |DMU|^T + 2 |A| |dv|), term for term.  ``dtype=np.float64`` runs the same closed form in float64.
"""
import functools

import numpy as np

import svgp_reference as SR
from pass2_reference import KID, LD, worst_ratio
from sgpmc_reference import low, sym
from svgp_reference import _f64, _forward, _kernel_bwd, gauss_hermite, log_ndtr

MUTATIONS = ("clamp_dv", "all_classes", "no_eps", "one_class_Sp", "fold_sign", "fold_factor", "dmu_datum_major")
ROWS_KEYS = ("out", "G", "g", "dmu", "dv")
TAIL_KEYS = ("F", "data", "prior", "vbar", "bbar", "Kuubar", "kappabar")
GRAD_KEYS = ("g_V", "g_ls", "g_sf2", "g_Z")
FLOOR_SCALE = 2.0 ** -40
EPS = 1e-3
TINY = float(np.finfo(np.float64).tiny)   # no float64 result is held below the format's smallest normal number (sgpmc_lik_reference)


def robustmax(y, MU, var, a_MU, a_v, eps, F, mutate=None):
    """Per datum ((ell, dMU (N x C), dvar, p), (a_ell, a_dMU, a_dvar)) of the robust-max likelihood under N(MU_n, var_n I)."""
    N, C = MU.shape
    x, w = gauss_hermite(F)
    yi = np.asarray(_f64(y)).astype(np.int64)
    rows = np.arange(N)
    sd = np.sqrt(var)
    D = (MU[rows, yi][:, None] - MU) / sd[:, None]                       # N x C; 0 in column y_n
    mask = np.ones((N, C), F)
    if mutate != "all_classes":
        mask[rows, yi] = 0
    z = x[None, :, None] + D[:, None, :]                                 # N x 20 x C
    lp = log_ndtr(z, F)
    P = w[None, :] * np.exp((lp * mask[:, None, :]).sum(2))              # N x 20
    p = P.sum(1)
    r = np.exp(-z * z / 2 - np.log(2 * np.arccos(F(-1))) / 2 - lp)       # phi / Phi
    R = (P[:, :, None] * r * mask[:, None, :]).sum(1)                    # d p / d delta_c  (>= 0)
    l1, l0 = np.log1p(-F(eps)), np.log(F(eps) / F(C - 1))
    kap = l1 - l0
    if mutate == "no_eps":                                               # the (1 - p) log(eps / (C - 1)) term dropped
        l0, kap = F(0), l1
    ell = p * l1 + (1 - p) * l0
    dD = kap * R                                                         # d ell / d delta_c
    dMU = -dD / sd[:, None]
    dMU[rows, yi] = dMU[rows, yi] + dD.sum(1) / sd
    dvar = -(dD * D).sum(1) / (2 * var)
    # ---- scales (float64) ----
    sd6, var6, D6, R6, P6, r6, m6, k6 = _f64(sd), _f64(var), np.abs(_f64(D)), _f64(R), _f64(P), _f64(r), _f64(mask), abs(float(kap))
    a_D = (a_MU[rows, yi][:, None] + a_MU) / sd6[:, None] + D6 * (a_v / (2 * var6))[:, None]
    pr = P6[:, :, None] * r6 * m6[:, None, :]                            # N x 20 x C
    H = np.einsum("nic,nid->ncd", pr, r6 * m6[:, None, :])               # |d2 p / d delta_c d delta_d| bound: P r_c r_d ...
    H[:, np.arange(C), np.arange(C)] += (pr * np.abs(_f64(z) + r6)).sum(1)   # ... and P r_c |z_c + r_c| on the diagonal
    a_R = np.einsum("ncd,nd->nc", H, a_D)
    # A quadrature term P_i that lands below the smallest normal number is held by float64 to an ABSOLUTE 2^-1074 only, and every
    # output multiplies it by a factor that may be large (dv: kappa r_ic delta_c / (2 var), 1e7 at a saturated datum with a small
    # variance); so is a phi / Phi that underflows beside a P_i of order one.  So TINY enters each scale carried through those
    # factors, with amp_c = sum_i r_ic for the first case and p = sum_i P_i for the second.
    amp = (r6 * m6[:, None, :]).sum(1)
    a_ell = abs(float(l0)) + k6 * _f64(p) + k6 * (R6 * a_D).sum(1) + TINY * (1 + k6 * len(w))
    a_dD = k6 * a_R
    a_dMU = (a_dD + k6 * R6 + TINY * k6 * (amp + _f64(p)[:, None])) / sd6[:, None] + (k6 * R6 / sd6[:, None]) * (a_v / (2 * var6))[:, None]
    a_dMU[rows, yi] = a_dMU.sum(1) - a_dMU[rows, yi] * (1 - m6[rows, yi])
    a_dvar = ((a_dD * D6 + k6 * R6 * a_D + (k6 * R6 + TINY * k6 * (amp + _f64(p)[:, None])) * D6).sum(1) + k6 * (R6 * D6).sum(1) * a_v / var6) / (2 * var6)
    return (ell, dMU, dvar, p), (a_ell, a_dMU + TINY, a_dvar + TINY)


def _c(a, F):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return (a if a.dtype == LD else a.astype(np.float64)).astype(F)


def reference(X, y, Z, ls, sf2, jitter, kernel, V, eps=EPS, dtype=LD, mutate=None, grads=True):
    """(ref, A) of every output of the two entry points (ROWS_KEYS, TAIL_KEYS, ref["mu"] (C x N), ref["var"], ref["floored"], ref["p"])
    and with ``grads`` the complete gradient (GRAD_KEYS) in row space beside the reuse route ("reuse_" + GRAD_KEYS, "reuse_Kfubar",
    "row_Kfubar", "row_Kuubar", "T_in")."""
    assert mutate is None or mutate in MUTATIONS
    F = dtype
    kid = KID[kernel]
    X, y, Z, ls, V = _c(X, F), _c(y, F).reshape(-1), _c(Z, F), _c(ls, F).reshape(-1), _c(V, F)
    sf2 = F(_c(sf2, F))
    N, M, C = X.shape[0], Z.shape[0], V.shape[0]
    f = _forward(X, Z, ls, sf2, V[0], np.zeros((M, M), F), jitter, kid, F)
    Am, Li, L, aA, aLi, var, a_v = f["A"], f["Li"], f["L"], f["aA"], f["aLi"], f["v"], f["a_v"]
    aV = np.abs(_f64(V))
    MU, a_MU = Am.T @ V.T, aA.T @ aV.T
    floor = sf2 * F(FLOOR_SCALE)
    floored = var < floor
    a_vf = np.where(floored, 0.0, a_v)
    (ell, dMU, e_v, p), (a_ell, a_dMU, a_ev) = robustmax(y, MU, np.where(floored, floor, var), a_MU, a_vf, eps, F, mutate)
    e_v, a_ev = np.where(floored, F(0), e_v), np.where(floored, 0.0, a_ev)
    dv_used = np.minimum(e_v, 0) if mutate == "clamp_dv" else e_v
    g, a_g = (Am @ dMU).T, (aA @ a_dMU).T                               # C x M
    G, a_G = (Am * dv_used) @ Am.T, (aA * a_ev) @ aA.T
    LOG2PI = np.log(2 * np.arccos(F(-1)))
    data, prior = ell.sum(), -(V * V).sum() / 2 - F(M * C) / 2 * LOG2PI
    a_prior = float((V * V).sum() / 2 + F(M * C) / 2 * LOG2PI)
    classes = range(1) if mutate == "one_class_Sp" else range(C)
    chol_adj = sum((sym(low(np.outer(V[c], g[c]))) for c in classes), np.zeros((M, M), F))
    a_chol = sum((sym(low(np.outer(aV[c], a_g[c]))) for c in range(C)), np.zeros((M, M)))
    Sp, a_Sp = G - chol_adj, a_G + a_chol
    ref = {"out": np.array([data, F(0), e_v.sum()]), "G": G, "g": g, "dmu": dMU.T.copy(), "dv": e_v, "F": data + prior, "data": data,
           "prior": prior, "vbar": g - V, "bbar": (Li.T @ V.T).T, "Kuubar": Li.T @ Sp @ Li, "kappabar": e_v.sum() / max(N, 1),
           "mu": MU.T.copy(), "var": var, "floored": floored, "p": p}
    A = {"out": np.array([a_ell.sum(), 1.0, a_ev.sum()]), "G": a_G, "g": a_g, "dmu": a_dMU.T.copy(), "dv": a_ev,
         "F": a_ell.sum() + a_prior, "data": a_ell.sum(), "prior": a_prior, "vbar": a_g + aV, "bbar": (aLi.T @ aV.T).T,
         "Kuubar": aLi.T @ a_Sp @ aLi, "kappabar": a_ev.sum() / max(N, 1), "mu": a_MU.T.copy(), "var": a_v}
    if not grads:
        return ref, A
    # ---- row space ----
    Abar, a_Abar = V.T @ dMU.T - 2 * Am * e_v, aV.T @ a_dMU.T + 2 * aA * a_ev       # M x N
    Kufbar, a_Kufbar = Li.T @ Abar, aLi.T @ a_Abar
    Lbar, a_Lbar = -np.tril(Kufbar @ Am.T), np.tril(a_Kufbar @ aA.T)
    Kuubar_row = sym(Li.T @ low(L.T @ Lbar) @ Li)
    a_Kuubar = sym(aLi.T @ low(np.abs(_f64(L)).T @ a_Lbar) @ aLi)
    (s_uf, l_uf, z_uf), (as_uf, al_uf, az_uf) = _kernel_bwd(X, Z, ls, sf2, Kufbar.T, a_Kufbar.T, kid, kid, F, False)
    (s_uu, l_uu, z_uu), (as_uu, al_uu, az_uu) = _kernel_bwd(Z, Z, ls, sf2, Kuubar_row, a_Kuubar, kid, kid, F, False)
    ref.update(g_V=g - V, g_sf2=s_uf + s_uu + e_v.sum(), g_ls=l_uf + l_uu, g_Z=z_uf + 2 * z_uu, row_Kfubar=Kufbar.T,
               row_Kuubar=Kuubar_row)
    A.update(g_V=a_g + aV, g_sf2=as_uf + as_uu + a_ev.sum(), g_ls=al_uf + al_uu, g_Z=az_uf + 2 * az_uu, row_Kfubar=a_Kufbar.T,
             row_Kuubar=a_Kuubar)
    # ---- the reuse route: the tail's Kuubar and ONE factored pass 2 on the folded T_in ----
    T = Am.T / sf2                                                      # unit amplitude, N x M
    DMU = dMU                                                           # N x C
    if mutate == "dmu_datum_major":                                     # the C x N class-major array read as if it were N x C
        DMU = np.ascontiguousarray(dMU.T).reshape(N, C)
    fold = DMU @ V / (sf2 if mutate == "fold_factor" else 2 * sf2)
    T_in = dv_used[:, None] * T + (fold if mutate == "fold_sign" else -fold)
    Kfubar = sf2 * (T_in @ (-2 * np.eye(M, dtype=F))) @ Li
    (r_uf, rl_uf, rz_uf), _ = _kernel_bwd(X, Z, ls, sf2, Kfubar, a_Kufbar.T, kid, kid, F, False)
    (r_uu, rl_uu, rz_uu), _ = _kernel_bwd(Z, Z, ls, sf2, ref["Kuubar"], a_Kuubar, kid, kid, F, False)
    ref.update(T_in=T_in, reuse_Kfubar=Kfubar, reuse_g_V=ref["vbar"], reuse_g_sf2=r_uf + r_uu + ref["kappabar"] * N,
               reuse_g_ls=rl_uf + rl_uu, reuse_g_Z=rz_uf + 2 * rz_uu)
    for k in GRAD_KEYS:
        A["reuse_" + k] = A[k]
    A["reuse_Kfubar"] = A["row_Kfubar"]
    A["T_in"] = (aA.T * a_ev[:, None] + a_dMU @ aV / 2) / float(sf2)
    return ref, A


def F_of(X, y, Z, ls, sf2, jitter, kernel, V, eps=EPS, dtype=LD):
    """F alone (finite differences of the reference's own density)."""
    return reference(X, y, Z, ls, sf2, jitter, kernel, V, eps, dtype, grads=False)[0]["F"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the cells of tests/test_sgpmc_mc_gpu.py (and of the CPU tests that measure its tolerance)
# ---------------------------------------------------------------------------------------------------------------------------------
# (N, M, d, C): each the smallest shape reaching its branch -- see the GPU test's docstring
CELLS = [(1, 1, 1, 2), (63, 5, 1, 3), (255, 64, 2, 3), (256, 64, 2, 3), (257, 65, 3, 4), (300, 129, 9, 5), (200, 130, 32, 3),
         (600, 300, 2, 16), (65537, 5, 1, 3)]
# (kernel, scale of V): rbf on every cell, the Matern kernels on two, V = 0 / N(0, 1) / 30 N(0, 1)
COMBOS = {
    (1, 1, 1, 2): [("rbf", 1.0)],
    (63, 5, 1, 3): [("rbf", 0.0), ("rbf", 1.0), ("rbf", 30.0), ("matern32", 1.0)],
    (255, 64, 2, 3): [("rbf", 1.0), ("rbf", 30.0)],
    (256, 64, 2, 3): [("rbf", 1.0), ("rbf", 0.0)],
    (257, 65, 3, 4): [("rbf", 1.0), ("matern52", 1.0)],
    (300, 129, 9, 5): [("rbf", 1.0)],
    (200, 130, 32, 3): [("rbf", 1.0)],
    (600, 300, 2, 16): [("rbf", 1.0)],
    (65537, 5, 1, 3): [("rbf", 1.0)],
}


@functools.lru_cache(maxsize=None)
def cell_inputs(N, M, d, C, vscale):
    """Inputs of a cell (float64 numpy, read-only): X, Z, ls, sf2, jitter of ``svgp_reference.cell_inputs`` (the first min(3, M, N)
    rows of X are rows of Z: the variance floor; (63, 5, 1) is its ill-conditioned cell, lengthscale 3.5 spacings), V = vscale x
    standard normal, and labels that are the argmax of the latent means under the UNSCALED V with a third of them redrawn uniformly
    (so that wrong data, dv > 0, sit beside right ones, dv < 0) -- over the classes 0 .. C-2 only: class C-1 has no datum."""
    base = SR.cell_inputs(N, M, d, "gaussian")
    rng = np.random.default_rng(13 + 1000003 * N + 1009 * M + 17 * d + C)
    X = np.array(base["X"])
    if (N, M, d) == SR.ILL_CELL:
        # 3.5 spacings pin the latent functions between the inducing inputs: var_n ~ the jitter there, every datum saturates and all
        # derivatives vanish.  The rows that do not sit on an inducing input are spread to three times the box, so that this cell,
        # too, has data with a variance of the order of sf2 (K_uu, and with it the conditioning, is untouched).
        k = min(3, M, N)
        mid = 0.5 * (X.min(0) + X.max(0))
        X[k:] = mid + 3.0 * (X[k:] - mid)
    V1 = np.random.default_rng(11 + M + 101 * C).standard_normal((C, M))
    f = _forward(X, base["Z"], base["ls"], np.float64(base["sf2"]), V1[0], np.zeros((M, M)), base["jitter"], KID["rbf"], np.float64)
    MU = f["A"].T @ V1.T
    top = C - 1 if C > 2 else C                            # (two classes: both may get data)
    redraw = rng.uniform(size=N) < 1.0 / 3.0
    y = np.where(redraw, rng.integers(0, top, N), np.argmax(MU[:, :top], 1)).astype(np.float64)
    out = dict(X=X, y=y, Z=base["Z"], ls=base["ls"], sf2=base["sf2"], jitter=base["jitter"], V=vscale * V1, eps=EPS)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cell_reference(N, M, d, C, kernel, vscale, dtype=LD, mutate=None, grads=True):
    """(ref, A) of a cell, cached: several tests share a cell."""
    inp = cell_inputs(N, M, d, C, vscale)
    return reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["jitter"], kernel, inp["V"], inp["eps"], dtype=dtype,
                     mutate=mutate, grads=grads)


ALL_KEYS = ROWS_KEYS + TAIL_KEYS + GRAD_KEYS


def worst(got, ref, A, keys=ALL_KEYS):
    """{key: worst |got - ref| / A over the key's components}"""
    return {k: worst_ratio(got[k], ref[k], A[k]) for k in keys if k in got}


def measure_e64(N, M, d, C, kernel, vscale, grads=True):
    """The float64 level of a cell: the worst |float64 closed form - long double| / A over every compared component (both routes)."""
    ref, A = cell_reference(N, M, d, C, kernel, vscale, grads=grads)
    r64, _ = cell_reference(N, M, d, C, kernel, vscale, dtype=np.float64, grads=grads)
    keys = ALL_KEYS + (tuple("reuse_" + k for k in GRAD_KEYS) if grads else ())
    return max(worst({k: r64[k] for k in keys if k in r64}, ref, A, keys).values())
