"""Long-double reference of the multi-class (robust-max) SVGP bound (include/sgp.h: sgp_svgp_mc_elbo, sgp_svgp_mc_predict), of its five
gradient blocks, of the latent moments and of the class probabilities, with the condition scale of every component.

TEST INFRASTRUCTURE ONLY -- numpy ``longdouble`` on the host, in the style of tests/svgp_reference.py, whose forward pass, kernel
adjoint, Gauss-Hermite rule and log Phi it shares.  ([UPSTREAM] GPflow's MultiClass(RobustMax) under SVGP(num_latent_gps = C, whiten =
True), as recalled: nothing here is checked against it; the formulas below are the definition.)

C latent GPs share the kernel, Z and the minibatch; class c has q(u_c) = N(m_c, Ls_c Ls_c^T), Ls_c = tril(LS_c).  With K = K_uu + J I,
L = chol K, A = L^-1 K_ub:

    T_c = Ls_c^T A     mu_bc = A_b . m_c     v_bc = sf2 - |A_b|^2 + |T_c,b|^2     (raised to 2^-40 sf2, its derivative 0 there)
    z_ibc = (mu_by + sqrt(v_by) x_i - mu_bc) / sqrt(v_bc)  (c != y = y_b)     p_b = sum_i w_i prod_{c != y} Phi(z_ibc)
    ell_b = p_b log(1 - eps) + (1 - p_b) log(eps / (C - 1))     KL = sum_c KL(q(u_c) || N(0, I))     F = mean_b ell_b - KL / N
    with P_i = w_i prod Phi, r_ic = P_i phi(z_ic) / Phi(z_ic), kappa = log(1 - eps) - log(eps / (C - 1)):
    dmu_c = -kappa sum_i r_ic / sqrt(v_c)          dmu_y = kappa sum_c sum_i r_ic / sqrt(v_c)
    dv_c  = -kappa sum_i r_ic z_ic / (2 v_c)       dv_y  = kappa sum_c sum_i r_ic x_i / (2 sqrt(v_y) sqrt(v_c))
    g_m_c = A mubar_c - m_c / N      g_LS_c = tril(2 (A diag vbar_c) T_c^T) - (Ls_c - diag(1 / diag Ls_c)) / N
    Abar = sum_c [m_c mubar_c^T + 2 (Ls_c T_c - A) diag vbar_c]      direct d/dsf2 = sum_b sum_c vbar_bc
and from Abar on exactly svgp_reference's chain (Kubbar, Lbar, the Cholesky adjoint, the kernel contractions).

``reference`` returns (ref, A): A is the component-wise CONDITION SCALE -- the same sums with every factor replaced by its absolute
value, carried through z, the quadrature and exp() to first order (|d(phi/Phi)/dz| = r |z + r|), as svgp_reference and
sgpmc_mc_reference.robustmax do.  The scales are all-positive sums formed in float64.  ``dtype=np.float64`` runs the same closed form in
float64; ``mutate`` applies one deliberate defect (MUTATIONS) so that a test can show the comparison failing on it.
"""
import functools

import numpy as np

import svgp_reference as SR
from pass2_reference import KID, LD, worst_ratio
from sgpmc_mc_reference import EPS, FLOOR_SCALE, TINY
from sgpmc_reference import low, sym
from svgp_reference import _f64, _forward, _kernel_bwd, gauss_hermite, log_ndtr

MUTATIONS = ("shared_var", "no_x_term", "kl_class0", "abar_last", "m_datum_major", "floor_dv")
KEYS = ("elbo", "ell_sum", "kl", "g_m", "g_LS", "g_Z", "g_ls", "g_sf2")
PREDICT_KEYS = ("mean", "var", "probs")


def robustmax_pv(y, MU, V, a_MU, a_V, eps, F, mutate=None):
    """Per datum ((ell, dMU, dV, p), (a_ell, a_dMU, a_dV, a_p)) of the robust-max likelihood under independent N(MU_nc, V_nc);
    MU, V, a_MU, a_V: N x C (V already floored, a_V zero where it was)."""
    N, C = MU.shape
    x, w = gauss_hermite(F)
    yi = np.asarray(_f64(y)).astype(np.int64)
    rows = np.arange(N)
    if mutate == "shared_var":                                           # the labelled class's variance used for every class
        V = np.repeat(V[rows, yi][:, None], C, 1)
    sd = np.sqrt(V)
    sdy, Vy = sd[rows, yi], V[rows, yi]
    mask = np.ones((N, C), F)
    mask[rows, yi] = 0
    D = (MU[rows, yi][:, None] - MU) / sd                                # N x C
    Bc = sdy[:, None] / sd                                               # N x C
    z = D[:, None, :] + Bc[:, None, :] * x[None, :, None]                # N x 20 x C
    lp = log_ndtr(z, F)
    P = w[None, :] * np.exp((lp * mask[:, None, :]).sum(2))              # N x 20
    p = P.sum(1)
    r = np.exp(-z * z / 2 - np.log(2 * np.arccos(F(-1))) / 2 - lp)       # phi / Phi
    q = P[:, :, None] * r * mask[:, None, :]                             # r_ic of the docstring, N x 20 x C
    R = q.sum(1)
    Xs = (q * x[None, :, None]).sum(1)
    l1, l0 = np.log1p(-F(eps)), np.log(F(eps) / F(C - 1))
    kap = l1 - l0
    ell = p * l1 + (1 - p) * l0
    dMU = -kap * R / sd
    dMU[rows, yi] = kap * (R / sd).sum(1)
    dV = -kap * (q * z).sum(1) / (2 * V)
    dV[rows, yi] = 0 if mutate == "no_x_term" else kap * (Xs / sd).sum(1) / (2 * sdy)
    # ---- scales (float64) ----
    sd6, V6, D6, B6, x6, w6 = _f64(sd), _f64(V), np.abs(_f64(D)), _f64(Bc), np.abs(_f64(x)), _f64(w)
    sdy6, Vy6, z6, r6, q6, m6, k6 = _f64(sdy), _f64(Vy), _f64(z), _f64(r), _f64(q), _f64(mask), abs(float(kap))
    relc, rely = a_V / (2 * V6), (a_V[rows, yi] / (2 * Vy6))[:, None]     # relative scale of sqrt(v_c), sqrt(v_y)
    a_z = ((a_MU[rows, yi][:, None] + a_MU) / sd6 + D6 * relc)[:, None, :] + (B6 * (1 + relc + rely))[:, None, :] * x6[None, :, None]
    rm = r6 * m6[:, None, :]
    # |d q_ic| <= q_ic (sum_d r_id a_z_id + |z_ic + r_ic| a_z_ic) + q_ic; a term P_i or phi / Phi below the smallest normal number is
    # held to an absolute 2^-1074 only (sgpmc_mc_reference.robustmax): TINY (r + 1) stands in for it
    a_q = q6 * ((rm * a_z).sum(2)[:, :, None] + np.abs(z6 + r6) * a_z + 1) + TINY * (rm + m6[:, None, :])
    a_p = _f64(p) + (q6 * a_z).sum((1, 2)) + TINY * len(w6)
    a_ell = abs(float(l0)) + k6 * a_p
    a_dMU = k6 * (a_q.sum(1) / sd6 + (_f64(R) / sd6) * relc)
    a_dMU[rows, yi] = a_dMU.sum(1) - a_dMU[rows, yi]
    a_dV = k6 * ((a_q * np.abs(z6) + q6 * a_z).sum(1) + 2 * (q6 * np.abs(z6)).sum(1) * relc) / (2 * V6)
    qx, a_qx = (q6 * x6[None, :, None]).sum(1), (a_q * x6[None, :, None]).sum(1)
    a_dV[rows, yi] = k6 * ((a_qx + qx * (relc + rely)) / sd6).sum(1) / (2 * sdy6)
    return (ell, dMU, dV, p), (a_ell, a_dMU + TINY, a_dV + TINY, a_p)


def _c(a, F):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return (a if a.dtype == LD else a.astype(np.float64)).astype(F)


def _moments(X, Z, ls, sf2, m, Ls, jitter, kid, F, mutate=None):
    """The shared forward: svgp_reference._forward for L, L^-1, A and their scales, then T_c, MU (B x C), V (B x C) per class."""
    C, M = m.shape
    f = _forward(X, Z, ls, sf2, m[0], Ls[0], jitter, kid, F)
    Am, aA = f["A"], f["aA"]
    m_used = m
    if mutate == "m_datum_major":                                        # the C x M class-major array read as if it were M x C
        m_used = np.ascontiguousarray(m.reshape(M, C).T)
    aLs = _f64(np.abs(Ls))
    T = [Ls[c].T @ Am for c in range(C)]
    aT = [aLs[c].T @ aA for c in range(C)]
    MU, a_MU = Am.T @ m_used.T, aA.T @ np.abs(_f64(m)).T
    sA, a_sA = (Am * Am).sum(0), (aA * aA).sum(0)
    V = np.stack([sf2 - sA + (T[c] * T[c]).sum(0) for c in range(C)], 1)
    a_V = np.stack([float(sf2) + a_sA + (aT[c] * aT[c]).sum(0) for c in range(C)], 1)
    f.update(T=T, aT=aT, aLs=aLs, MU=MU, a_MU=a_MU, V=V, a_V=a_V)
    return f


def reference(X, y, Z, ls, sf2, jitter, kernel, m, LS, N_total, eps=EPS, dtype=LD, mutate=None, grads=True):
    """(ref, A) of sgp_svgp_mc_elbo: KEYS, and ref["mu"], ref["v"] (B x C, v as formed), ref["floored"], ref["dmu"], ref["dv"], ref["p"]."""
    assert mutate is None or mutate in MUTATIONS
    F = dtype
    kid = KID[kernel]
    X, y, Z, ls, m = _c(X, F), _c(y, F).reshape(-1), _c(Z, F), _c(ls, F).reshape(-1), _c(m, F)
    Ls = np.tril(_c(LS, F))
    sf2 = F(_c(sf2, F))
    B, M, C, N = X.shape[0], Z.shape[0], m.shape[0], F(N_total)
    f = _moments(X, Z, ls, sf2, m, Ls, jitter, kid, F, mutate)
    Am, T, Li, L, aA, aT, aLi, aLs = f["A"], f["T"], f["Li"], f["L"], f["aA"], f["aT"], f["aLi"], f["aLs"]
    floor = sf2 * F(FLOOR_SCALE)
    floored = f["V"] < floor
    a_Vf = np.where(floored, 0.0, f["a_V"])
    (ell, e_mu, e_v, p), (a_ell, a_emu, a_ev, _) = robustmax_pv(y, f["MU"], np.where(floored, floor, f["V"]), f["a_MU"], a_Vf, eps, F, mutate)
    if mutate != "floor_dv":
        e_v, a_ev = np.where(floored, F(0), e_v), np.where(floored, 0.0, a_ev)
    am = np.abs(_f64(m))
    dg = np.stack([np.diagonal(Ls[c]) for c in range(C)])
    klc = ((m * m).sum(1) + (Ls * Ls).sum((1, 2)) - M - 2 * np.log(dg).sum(1)) / 2
    a_klc = _f64((m * m).sum(1) + (Ls * Ls).sum((1, 2)) + M + 2 * np.abs(np.log(dg)).sum(1)) / 2
    kl = klc[0] if mutate == "kl_class0" else klc.sum()
    a_kl = float(a_klc.sum())
    ref = {"elbo": ell.sum() / B - kl / N, "ell_sum": ell.sum(), "kl": kl, "mu": f["MU"], "v": f["V"], "floored": floored, "dmu": e_mu,
           "dv": e_v, "p": p}
    A = {"elbo": a_ell.sum() / B + a_kl / float(N), "ell_sum": a_ell.sum(), "kl": a_kl, "mu": f["a_MU"], "v": f["a_V"], "dmu": a_emu, "dv": a_ev}
    if not grads:
        return ref, A
    mub, vb, a_mub, a_vb = e_mu / B, e_v / B, a_emu / B, a_ev / B                 # B x C
    ref["g_m"], A["g_m"] = (Am @ mub).T - m / N, (aA @ a_mub).T + am / float(N)
    g_LS, a_gLS = np.zeros((C, M, M), F), np.zeros((C, M, M))
    Abar, a_Abar = np.zeros_like(Am), np.zeros_like(aA)
    for c in range(C):
        G, aG = (Am * vb[:, c]) @ T[c].T, (aA * a_vb[:, c]) @ aT[c].T
        g_LS[c] = np.tril(2 * G) - (Ls[c] - np.diag(1 / dg[c])) / N
        a_gLS[c] = np.tril(2 * aG) + (aLs[c] + np.diag(1 / np.abs(_f64(dg[c])))) / float(N)
        term = np.outer(m[c], mub[:, c]) + 2 * (Ls[c] @ T[c] - Am) * vb[:, c]
        Abar = term if mutate == "abar_last" else Abar + term
        a_Abar = a_Abar + np.outer(am[c], a_mub[:, c]) + 2 * (aLs[c] @ aT[c] + aA) * a_vb[:, c]
    ref["g_LS"], A["g_LS"] = g_LS, a_gLS
    Kubbar, a_Kubbar = Li.T @ Abar, aLi.T @ a_Abar
    Lbar, a_Lbar = -np.tril(Kubbar @ Am.T), np.tril(a_Kubbar @ aA.T)
    Kuubar = sym(Li.T @ low(L.T @ Lbar) @ Li)
    a_Kuubar = sym(aLi.T @ low(np.abs(_f64(L)).T @ a_Lbar) @ aLi)
    (s_ub, l_ub, z_ub), (as_ub, al_ub, az_ub) = _kernel_bwd(X, Z, ls, sf2, Kubbar.T, a_Kubbar.T, kid, kid, F, False)
    (s_uu, l_uu, z_uu), (as_uu, al_uu, az_uu) = _kernel_bwd(Z, Z, ls, sf2, Kuubar, a_Kuubar, kid, kid, F, False)
    ref["g_sf2"], A["g_sf2"] = s_ub + s_uu + vb.sum(), as_ub + as_uu + a_vb.sum()
    ref["g_ls"], A["g_ls"] = l_ub + l_uu, al_ub + al_uu
    ref["g_Z"], A["g_Z"] = z_ub + 2 * z_uu, az_ub + 2 * az_uu
    return ref, A


def predict_reference(Xs, Z, ls, sf2, jitter, kernel, m, LS, eps=EPS, dtype=LD):
    """(ref, A) of sgp_svgp_mc_predict at the rows of Xs: "mean", "var" (C x T, var as formed) and "probs" (T x C)."""
    F = dtype
    Xs, Z, ls, m = _c(Xs, F), _c(Z, F), _c(ls, F).reshape(-1), _c(m, F)
    Ls = np.tril(_c(LS, F))
    sf2 = F(_c(sf2, F))
    C = m.shape[0]
    f = _moments(Xs, Z, ls, sf2, m, Ls, jitter, KID[kernel], F)
    floor = sf2 * F(FLOOR_SCALE)
    floored = f["V"] < floor
    Vf, a_Vf = np.where(floored, floor, f["V"]), np.where(floored, 0.0, f["a_V"])
    probs, a_probs = np.zeros(f["MU"].shape, F), np.zeros(f["MU"].shape)
    e, o = F(eps), F(eps) / F(C - 1)
    for c in range(C):
        (_, _, _, p), (_, _, _, a_p) = robustmax_pv(np.full(Xs.shape[0], float(c)), f["MU"], Vf, f["a_MU"], a_Vf, eps, F)
        probs[:, c] = (1 - e) * p + o * (1 - p)
        a_probs[:, c] = float(1 - e) * a_p + float(o) * (1 + a_p)
    return ({"mean": f["MU"].T.copy(), "var": f["V"].T.copy(), "probs": probs},
            {"mean": f["a_MU"].T.copy(), "var": f["a_V"].T.copy(), "probs": a_probs})


def F_of(X, y, Z, ls, sf2, jitter, kernel, m, LS, N_total, eps=EPS, dtype=LD):
    """The bound alone (finite differences of the reference's own value)."""
    return reference(X, y, Z, ls, sf2, jitter, kernel, m, LS, N_total, eps, dtype, grads=False)[0]["elbo"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the cells of tests/test_svgp_mc_gpu.py (and of the CPU tests that measure its tolerance)
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, M, d, C): each the smallest shape reaching its branch -- see the GPU test's docstring
CELLS = [(1, 1, 1, 2), (63, 5, 1, 3), (64, 64, 2, 3), (65, 65, 3, 4), (257, 128, 8, 3), (300, 129, 9, 5), (200, 130, 32, 3),
         (600, 300, 2, 16), (16385, 5, 1, 3)]
COMBOS = {cell: ["rbf"] for cell in CELLS}                   # rbf on every cell, the Matern kernels on two
COMBOS[(63, 5, 1, 3)] = ["rbf", "matern32"]
COMBOS[(65, 65, 3, 4)] = ["rbf", "matern52"]
PREDICT_CELL = (300, 129, 9, 5)
FLOOR_CELL = (65, 65, 3, 4)
FLOOR_JITTER = 1e-13        # below the floor 2^-40 sf2 = 1.2e-12: sf2 - |A_b|^2 of a datum on an inducing input is ~ the jitter
FLOOR_LS_SCALE = 1e-25      # ... and |T_c,b|^2 of the class whose factor is scaled by this adds nothing to it


@functools.lru_cache(maxsize=None)
def cell_inputs(B, M, d, C, floor=False):
    """Inputs of a cell (float64 numpy, read-only): X, Z, ls, sf2, jitter, N_total of ``svgp_reference.cell_inputs`` (the first
    min(3, M, B) rows of X are rows of Z; (63, 5, 1) is its ill-conditioned cell, lengthscale 3.5 spacings).  m: C x M standard normal.
    LS_c = s_c I + tril(0.15 N(0, 1)) with s_c from 0.5 to 1.5 over the classes: the factors differ, their off-diagonal entries have
    both signs, and the per-class variances of a datum near an inducing input differ by up to 9.  Labels: the arg-max of the latent
    means over the classes 0 .. C-2 (class C-1 has no datum when C > 2) with a third redrawn uniformly over them, so that data whose
    labelled class leads sit beside data whose labelled class trails.  ``floor``: the jitter lowered to FLOOR_JITTER and LS_1 scaled by
    FLOOR_LS_SCALE, so that class 1's variance of the data on inducing inputs falls below the floor; the first of them is labelled 1."""
    base = SR.cell_inputs(B, M, d, "gaussian")
    rng = np.random.default_rng(29 + 1000003 * B + 1009 * M + 17 * d + C)
    m = rng.standard_normal((C, M))
    s = 0.5 + np.arange(C) / (C - 1.0)
    LS = np.tril(0.15 * rng.standard_normal((C, M, M)), -1) + s[:, None, None] * np.eye(M)
    jitter = base["jitter"]
    if floor:
        LS[1] *= FLOOR_LS_SCALE
        jitter = FLOOR_JITTER
    f = _forward(np.array(base["X"]), base["Z"], base["ls"], np.float64(base["sf2"]), m[0], LS[0], jitter, KID["rbf"], np.float64)
    MU = f["A"].T @ m.T
    top = C - 1 if C > 2 else C
    redraw = rng.uniform(size=B) < 1.0 / 3.0
    y = np.where(redraw, rng.integers(0, top, B), np.argmax(MU[:, :top], 1)).astype(np.float64)
    if floor:
        # the floored class is the LABELLED one of the first datum on an inducing input: dv_y = kappa sum_c X_c / (2 sqrt(v_y) sqrt(v_c))
        # carries 1 / sqrt(v_y) there (the non-labelled classes' dv vanishes with phi / Phi at |z| ~ 1e6 whether it is zeroed or not)
        y[0] = 1.0
    out = dict(X=base["X"], y=y, Z=base["Z"], ls=base["ls"], sf2=base["sf2"], jitter=jitter, m=m, LS=LS, N_total=base["N_total"], eps=EPS)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _ref_of(inp, kernel, **kw):
    return reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["jitter"], kernel, inp["m"], inp["LS"], inp["N_total"],
                     inp["eps"], **kw)


@functools.lru_cache(maxsize=None)
def cell_reference(B, M, d, C, kernel, dtype=LD, mutate=None, grads=True, floor=False):
    """(ref, A) of a cell, cached: several tests share a cell."""
    return _ref_of(cell_inputs(B, M, d, C, floor), kernel, dtype=dtype, mutate=mutate, grads=grads)


@functools.lru_cache(maxsize=None)
def predict_cell_reference(kernel, T, dtype=LD):
    inp = cell_inputs(*PREDICT_CELL)
    return predict_reference(inp["X"][:T], inp["Z"], inp["ls"], inp["sf2"], inp["jitter"], kernel, inp["m"], inp["LS"], inp["eps"], dtype=dtype)


def worst(got, ref, A, keys=KEYS):
    """{key: worst |got - ref| / A over the key's components}; ``got`` maps the keys to arrays / tensors / numbers."""
    return {k: worst_ratio(got[k], ref[k], A[k]) for k in keys if k in got}
