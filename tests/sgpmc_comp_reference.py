"""Long-double reference of SGPMC with a composite kernel, a white-noise term and a linear mean function (include/sgp.h:
sgp_sgpmc_comp_rows, sgp_sgpmc_comp_bwd, with sgp_sgpmc_lik_tail and sgp_kuu_bwd behind them) and of the complete gradient.

TEST INFRASTRUCTURE ONLY -- numpy ``longdouble`` on the host, in the style of tests/sgpmc_lik_reference.py, whose likelihood layer,
Gauss-Hermite rule, ``low`` / ``sym`` and cell geometry it imports.  The composite kernel and its parameter derivatives are restated
here in long double (``comp_k``).  With K = k(Z, Z) + (J + white) I, L = chol(K), A = L^-1 k(Z, X) (M x N, column n is a_n):

    mu = A^T v + (X c + c0)     var = kdiag + white - colsum(A o A)  (raised to 2^-40 k_nn, its derivative 0 there)
    rows:  out = [sum ell | sum d ell / d s2 | sum dv]   g = A dmu   G = (A diag(dv)) A^T   dmu, dv, mu, var   T_out = diag(dv) A^T
    tail:  F = sum ell - v.v / 2 - M/2 log 2 pi          vbar = g - v     bbar = L^-T v     Kuubar = L^-T (G - sym(low(v g^T))) L^-1

The complete gradient dF / d{v, block, white, s2, c, c0} is formed IN ROW SPACE, as the SVGP reference forms its own:

    Abar = v dmu^T - 2 A diag(dv)     Kufbar = L^-T Abar     Lbar = -tril(Kufbar A^T)     Kuubar' = sym(L^-T low(L^T Lbar) L^-1)
    g_block[k] = sum(Kufbar o dk_uf/dtheta_k) + sum(Kuubar' o dk_uu/dtheta_k) + sum dv [theta_k an amp2 slot]
    g_white = tr Kuubar' + sum dv     g_c = X^T dmu     g_c0 = sum dmu     g_s2 = sum d ell / d s2     g_v = g - v

-- WITHOUT the reuse arguments of the device code, which are restated beside it under "reuse_*": G = -S^T S, the tail's Kuubar
contracted as it is (unsymmetrised), and the N-side adjoint Kfubar = -2 T_in L^-1 + dmu w^T with T_in = diag(dv) T.  ``bwd_g_blk`` is
what sgp_sgpmc_comp_bwd alone returns.  ``mutate`` breaks one thing at a time (MUTATIONS).

``reference`` returns (ref, A): A is the CONDITION SCALE of each component (the same sums with every factor replaced by its absolute
value, carried to first order through the likelihood); the comparison is |got - ref| <= tol * A.  ``dtype=np.float64`` runs the same
closed form in float64 (``measure_e64``)."""
import functools

import numpy as np

import sgpmc_lik_reference as LR
import svgp_reference as SR
from pass2_reference import LD, worst_ratio
from sgpmc_lik_reference import LIK, _c, expected_log_lik
from sgpmc_reference import chol_ld, low, sym, tri_inv_ld
from svgp_reference import _f64

EXPQUAD, MATERN32, MATERN52, RATQUAD, PERIODIC = 0, 1, 2, 3, 4
COMP_LEN = 33
MUTATIONS = ("no_white_in_kuu", "no_white_in_knn", "no_trace_term", "no_amp_kdiag_term", "mean_sign", "unscaled_T", "drop_row")
ROWS_KEYS = ("out", "G", "g", "dmu", "dv", "mu", "var", "T_out")
TAIL_KEYS = ("F", "data", "prior", "vbar", "bbar", "Kuubar", "s2bar", "kappabar")
GRAD_KEYS = ("bwd_g_blk", "g_v", "g_block", "g_white", "g_s2", "g_c", "g_c0")
ALL_KEYS = ROWS_KEYS + TAIL_KEYS + GRAD_KEYS
FLOOR_SCALE = 2.0 ** -40


def structure(block):
    """[(amp2 slot, [(type, ls slot, aux slot), ...]), ...] of a parameter block (include/sgp.h: SGP_COMP_*)."""
    b = np.asarray(block, dtype=np.float64)
    return [(1 + 8 * t, [(int(b[3 + 8 * t + 3 * f]), 4 + 8 * t + 3 * f, 5 + 8 * t + 3 * f) for f in range(int(b[2 + 8 * t]))])
            for t in range(int(b[0]))]


def param_slots(block):
    """The slots of the block that carry a derivative: amp2, every lengthscale, alpha of a ratquad and the period of a periodic factor."""
    out = []
    for amp, facs in structure(block):
        out.append(amp)
        for ty, ls, aux in facs:
            out += [ls] + ([aux] if ty in (RATQUAD, PERIODIC) else [])
    return out


def amp_slots(block):
    return [amp for amp, _ in structure(block)]


def _factor(ty, delta, r2, ls, aux, F):
    """(value, d / d ls, d / d aux) of one isotropic factor; delta: list of d difference matrices, r2 their squared sum."""
    zero = np.zeros_like(r2)
    if ty == EXPQUAD:
        k = np.exp(-r2 / (2 * ls * ls))
        return k, k * r2 / (ls * ls * ls), zero
    if ty in (MATERN32, MATERN52):
        a = np.sqrt((F(3) if ty == MATERN32 else F(5)) * r2) / ls
        e = np.exp(-a)
        if ty == MATERN32:
            return (1 + a) * e, a * a * e / ls, zero
        return (1 + a + a * a / 3) * e, a * a * (1 + a) * e / (3 * ls), zero
    if ty == RATQUAD:
        w = 1 + r2 / (2 * aux * ls * ls)
        k = np.exp(-aux * np.log(w))
        return k, k / w * r2 / (ls * ls * ls), k * ((w - 1) / w - np.log(w))
    pi = np.arccos(F(-1))
    S, dS = zero, zero
    for dj in delta:
        s = np.sin(pi * dj / aux)
        S = S + s * s
        dS = dS - np.sin(2 * pi * dj / aux) * pi * dj / (aux * aux)      # d sin^2(pi delta / T) / dT
    k = np.exp(-S / (2 * ls * ls))
    return k, k * S / (ls * ls * ls), -k * dS / (2 * ls * ls)


def comp_k(A, B, block, F, grads=False):
    """k(a_i, b_j) as an (na x nb) array of dtype F and, with ``grads``, {slot: dk / d block[slot]} for ``param_slots``."""
    delta = [A[:, None, j] - B[None, :, j] for j in range(A.shape[1])]
    r2 = delta[0] * delta[0]
    for dj in delta[1:]:
        r2 = r2 + dj * dj
    K, dK = np.zeros(r2.shape, F), {}
    for amp, facs in structure(block):
        vals = [_factor(ty, delta, r2, block[ls], block[aux], F) for ty, ls, aux in facs]
        prod = vals[0][0] if len(vals) == 1 else vals[0][0] * vals[1][0]
        K = K + block[amp] * prod
        if grads:
            dK[amp] = prod
            for f, (ty, ls, aux) in enumerate(facs):
                other = block[amp] * (vals[1 - f][0] if len(vals) == 2 else 1)
                dK[ls] = other * vals[f][1]
                if ty in (RATQUAD, PERIODIC):
                    dK[aux] = other * vals[f][2]
    return (K, dK) if grads else K


def _contract(Kbar, Kabs, dK, slots, F):
    return (np.array([np.einsum("ij,ij->", Kbar, dK[s]) for s in slots], F),
            np.array([np.einsum("ij,ij->", Kabs, np.abs(_f64(dK[s]))) for s in slots]))


def reference(X, y, Z, block, white, s2, c, c0, jitter, lik, v, dtype=LD, mutate=None, grads=True):
    """(ref, A) of every output of the two entry points and of the tail (ROWS_KEYS, TAIL_KEYS, ref["floored"], ref["cond"]) and, with
    ``grads``, the complete gradient in row space (GRAD_KEYS; g_block / bwd_g_blk over ``param_slots(block)``) beside the reuse route
    ("reuse_G", "reuse_Kfubar" against "row_Kfubar", "reuse_bwd_g_blk", "reuse_g_block", "reuse_g_white").  ``c`` (d) / ``c0``: the
    linear mean, None for none."""
    assert mutate is None or mutate in MUTATIONS
    F = dtype
    lik = LIK.get(lik, lik)
    X, y, Z, v = _c(X, F), _c(y, F).reshape(-1), _c(Z, F), _c(v, F).reshape(-1)
    blk = _c(block, F).reshape(-1)
    white, s2, J = F(_c(white, F)), F(_c(s2, F)), F(_c(jitter, F))
    N, M = X.shape[0], Z.shape[0]
    slots, amps = param_slots(_f64(blk)), amp_slots(_f64(blk))
    kdiag = sum(blk[a] for a in amps)
    Kuu, dKuu = comp_k(Z, Z, blk, F, True)
    Kuf, dKuf = comp_k(Z, X, blk, F, True)
    K = Kuu + (J + (0 if mutate == "no_white_in_kuu" else white)) * np.eye(M, dtype=F)
    L = chol_ld(K, F)
    Li = tri_inv_ld(L, F)
    Am = Li @ Kuf
    aLi = _f64(np.abs(Li))
    aA = aLi @ _f64(np.abs(Kuf))
    av = np.abs(_f64(v))
    mean, a_mean = np.zeros(N, F), np.zeros(N)
    if c is not None:
        cc, cc0 = _c(c, F).reshape(-1), F(_c(c0, F))
        mean, a_mean = X @ cc + cc0, _f64(np.abs(X)) @ _f64(np.abs(cc)) + abs(float(cc0))
        if mutate == "mean_sign":
            mean = -mean
    knn = kdiag + (0 if mutate == "no_white_in_knn" else white)
    mu, var = Am.T @ v + mean, knn - (Am * Am).sum(0)
    a_mu, a_v = aA.T @ av + a_mean, float(knn) + (aA * aA).sum(0)
    floor = knn * F(FLOOR_SCALE)
    floored = var < floor
    (ell, e_mu, e_v, e_s2, _), (a_ell, a_emu, a_ev, a_es2) = expected_log_lik(y, mu, np.where(floored, floor, var), a_mu, a_v, s2, lik, F)
    e_v, a_ev = np.where(floored | (e_v > 0), F(0), e_v), np.where(floored, 0.0, a_ev)
    e_s2, a_es2 = e_s2 * np.ones(N, F), a_es2 * np.ones(N)
    if mutate == "drop_row":
        for t in (ell, e_mu, e_v, e_s2):
            t[N - 1] = 0
    g, a_g = Am @ e_mu, aA @ a_emu
    G, a_G = (Am * e_v) @ Am.T, (aA * a_ev) @ aA.T
    LOG2PI = np.log(2 * np.arccos(F(-1)))
    data, prior = ell.sum(), -(v @ v) / 2 - F(M) / 2 * LOG2PI
    a_prior = float((v @ v) / 2 + F(M) / 2 * LOG2PI)
    Sp, a_Sp = G - sym(low(np.outer(v, g))), a_G + sym(low(np.outer(av, a_g)))
    ev64 = np.linalg.eigvalsh(_f64(K))
    ref = {"out": np.array([data, e_s2.sum(), e_v.sum()]), "G": G, "g": g, "dmu": e_mu, "dv": e_v, "mu": mu, "var": var,
           "T_out": e_v[:, None] * Am.T, "F": data + prior, "data": data, "prior": prior, "vbar": g - v, "bbar": Li.T @ v,
           "Kuubar": Li.T @ Sp @ Li, "s2bar": e_s2.sum(), "kappabar": e_v.sum() / max(N, 1), "floored": floored,
           "cond": float(ev64.max() / ev64.min()), "var_over_knn": float(_f64(var / knn).min()), "slots": slots}
    A = {"out": np.array([a_ell.sum(), a_es2.sum(), a_ev.sum()]), "G": a_G, "g": a_g, "dmu": a_emu, "dv": a_ev, "mu": a_mu, "var": a_v,
         "T_out": a_ev[:, None] * aA.T, "F": a_ell.sum() + a_prior, "data": a_ell.sum(), "prior": a_prior, "vbar": a_g + av,
         "bbar": aLi.T @ av, "Kuubar": aLi.T @ a_Sp @ aLi, "s2bar": a_es2.sum(), "kappabar": a_ev.sum() / max(N, 1)}
    if not grads:
        return ref, A
    # ---- row space ----
    Abar, a_Abar = np.outer(v, e_mu) - 2 * Am * e_v, np.outer(av, a_emu) + 2 * aA * a_ev
    Kufbar, a_Kufbar = Li.T @ Abar, aLi.T @ a_Abar
    Lbar, a_Lbar = -np.tril(Kufbar @ Am.T), np.tril(a_Kufbar @ aA.T)
    Kuubar_row = sym(Li.T @ low(L.T @ Lbar) @ Li)
    a_Kuubar = sym(aLi.T @ low(np.abs(_f64(L)).T @ a_Lbar) @ aLi)
    n_side, a_n = _contract(Kufbar, a_Kufbar, dKuf, slots, F)
    u_side, a_u = _contract(Kuubar_row, a_Kuubar, dKuu, slots, F)
    is_amp = np.array([s in amps for s in slots])
    diag_term = np.where(is_amp, F(0) if mutate == "no_amp_kdiag_term" else e_v.sum(), F(0))
    a_diag = np.where(is_amp, a_ev.sum(), 0.0)
    trace = F(0) if mutate == "no_trace_term" else np.trace(Kuubar_row)
    ref.update(bwd_g_blk=n_side, g_v=g - v, g_block=n_side + u_side + diag_term, g_white=trace + e_v.sum(), g_s2=e_s2.sum(),
               g_c=X.T @ e_mu, g_c0=e_mu.sum(), row_Kfubar=Kufbar.T, row_Kuubar=Kuubar_row)
    A.update(bwd_g_blk=a_n, g_v=a_g + av, g_block=a_n + a_u + a_diag, g_white=float(np.trace(a_Kuubar)) + a_ev.sum(), g_s2=a_es2.sum(),
             g_c=_f64(np.abs(X)).T @ a_emu, g_c0=a_emu.sum(), row_Kfubar=a_Kufbar.T, row_Kuubar=a_Kuubar)
    # ---- the reuse route: G = -S^T S, the tail's Kuubar as it is, the N-side adjoint from T_in = diag(dv) T ----
    S = np.sqrt(np.maximum(-e_v, 0))[:, None] * Am.T
    T_in = Am.T if mutate == "unscaled_T" else ref["T_out"]
    if mutate == "unscaled_T":
        ref["T_out"] = Am.T
    Kfubar = -2 * T_in @ Li + np.outer(e_mu, ref["bbar"])
    r_n, _ = _contract(Kfubar.T, a_Kufbar, dKuf, slots, F)
    r_u, _ = _contract(ref["Kuubar"], a_Kuubar, dKuu, slots, F)
    ref.update(reuse_G=-S.T @ S, reuse_Kfubar=Kfubar, reuse_bwd_g_blk=r_n, reuse_g_block=r_n + r_u + diag_term,
               reuse_g_white=np.trace(ref["Kuubar"]) + e_v.sum())
    A.update(reuse_G=a_G, reuse_Kfubar=A["row_Kfubar"], reuse_bwd_g_blk=a_n, reuse_g_block=A["g_block"], reuse_g_white=A["g_white"])
    if mutate == "unscaled_T":      # the device's gradient IS the reuse route: a wrong T_in shows there
        ref.update(bwd_g_blk=r_n, g_block=ref["reuse_g_block"])
    return ref, A


# ---------------------------------------------------------------------------------------------------------------------------------
# the cells of tests/test_sgpmc_comp_gpu.py (and of the CPU tests that measure its tolerance)
# ---------------------------------------------------------------------------------------------------------------------------------
# (N, M, d): each the smallest shape reaching its branch -- see the GPU test's docstring
CELLS = [(1, 1, 1), (63, 5, 1), (255, 64, 2), (256, 64, 2), (257, 65, 3), (300, 129, 8), (600, 200, 1), (65537, 5, 1)]
ILL_CELL = (63, 5, 1)
_ALL = ("gaussian", "bernoulli", "bernoulli_logit", "poisson")
# (likelihood, scale of v, extras): extras True = white 0.05 and the linear mean, False = white 0 and no mean
COMBOS = {
    (1, 1, 1): [("gaussian", 1.0, True)],
    (63, 5, 1): [(l, 1.0, False) for l in _ALL] + [("gaussian", 0.0, False), ("gaussian", 30.0, False)],
    (255, 64, 2): [("gaussian", 1.0, True)],
    (256, 64, 2): [("gaussian", 1.0, False)],
    (257, 65, 3): [(l, 1.0, True) for l in _ALL] + [("gaussian", 1.0, False)],
    (300, 129, 8): [("gaussian", 1.0, True)],
    (600, 200, 1): [("gaussian", 1.0, True), ("gaussian", 1.0, False)],
    (65537, 5, 1): [("gaussian", 1.0, True)],
}
WHITE = 0.05
MEAN_C, MEAN_C0 = 0.05, 0.1


def co2_block(var=(1.0, 0.7, 0.48, 0.5), ls=(1.2, 2.0, 1.0, 1.5, 0.8), alpha=1.5, period=7.3):
    """The structure of ``co2_sgpmc_kernel()`` -- Periodic x Matern52 + RatQuad + ExpQuad + Matern52 -- with lengthscales of 0.8 .. 2
    spacings of the cells' unit grid and a period of 7.3 spacings."""
    b = np.zeros(COMP_LEN)
    b[0] = 4
    b[1:9] = (var[0], 2, PERIODIC, ls[0], period, MATERN52, ls[1], 0)
    b[9:14] = (var[1], 1, RATQUAD, ls[2], alpha)
    b[17:22] = (var[2], 1, EXPQUAD, ls[3], 0)
    b[25:30] = (var[3], 1, MATERN52, ls[4], 0)
    return b


# the ill-conditioned cell: a trend of 3.5 spacings and next to nothing rough beside it (white = 0)
ILL_BLOCK = co2_block(var=(1e-4, 1e-4, 1.0, 1e-4), ls=(1.2, 2.0, 1.0, 3.5, 0.8))


@functools.lru_cache(maxsize=None)
def cell_inputs(N, M, d, lik, vscale, extras):
    """Inputs of a cell (float64 numpy, read-only): X, y, Z, v, jitter of ``sgpmc_lik_reference.cell_inputs`` (rows of X are rows of Z),
    the parameter block, white and the linear mean."""
    base = LR.cell_inputs(N, M, d, lik, vscale)
    out = dict(X=base["X"], y=base["y"], Z=base["Z"], v=base["v"], jitter=base["jitter"], s2=base["s2"],
               block=np.array(ILL_BLOCK if (N, M, d) == ILL_CELL else co2_block()), white=WHITE if extras else 0.0,
               c=np.full(d, MEAN_C) if extras else None, c0=MEAN_C0 if extras else None)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def reference_at(inp, lik, dtype=LD, mutate=None, grads=True):
    return reference(inp["X"], inp["y"], inp["Z"], inp["block"], inp["white"], inp["s2"], inp["c"], inp["c0"], inp["jitter"], lik, inp["v"],
                     dtype=dtype, mutate=mutate, grads=grads)


@functools.lru_cache(maxsize=None)
def cell_reference(N, M, d, lik, vscale, extras, dtype=LD, mutate=None, grads=True):
    """(ref, A) of a cell, cached: several tests share a cell."""
    return reference_at(cell_inputs(N, M, d, lik, vscale, extras), lik, dtype=dtype, mutate=mutate, grads=grads)


def all_cells():
    return [(*cell, l, s, x) for cell in CELLS for l, s, x in COMBOS[cell]]


def worst(got, ref, A, keys=ALL_KEYS):
    """{key: worst |got - ref| / A over the key's components}"""
    return {k: worst_ratio(got[k], ref[k], A[k]) for k in keys if k in got and got[k] is not None}


def measure_e64(N, M, d, lik, vscale, extras):
    """The float64 level of a cell: the worst |float64 closed form - long double| / A over every compared component."""
    ref, A = cell_reference(N, M, d, lik, vscale, extras)
    r64, _ = cell_reference(N, M, d, lik, vscale, extras, dtype=np.float64)
    return max(worst(r64, ref, A).values())
