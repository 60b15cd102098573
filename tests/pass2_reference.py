"""Long-double reference of the gradient pass (pass 2) and of the K_uu gradient, with the condition scale of every component.

TEST INFRASTRUCTURE ONLY -- numpy ``longdouble`` (x87 extended: eps 1.1e-19) on the host, rows walked in chunks, no device code.  It is
the yardstick tests/test_pass2_kernel.py holds sgp_suffstats_bwd, sgp_suffstats_bwd_factored(_ex) and sgp_kuu_bwd against.

The scalar whose gradient pass 2 delivers is

    L = sum(Phibar o (K_uf K_fu)) + bbar^T K_uf y + kappabar N sf2,          K_uf[m][n] = sf2 k'(r2[m][n]),
    r2[m][n] = sum_j ((z_mj - x_nj) / ls_j)^2,

so  Kbar_uf = dL/dK_uf = (Phibar + Phibar^T) K_uf + bbar y^T  -- Phibar need not be symmetric: the library symmetrises it to
(Phibar + Phibar^T) / 2 in its prologue, which is the same Kbar_uf -- and with  E = Kbar_uf o sf2 dk'/dr2

    g_sf2    = sum(Kbar_uf o k') + kappabar N
    g_ls[j]  = sum_{m,n} E (-2 (z_mj - x_nj)^2 / ls_j^3)
    g_Z[m,j] = sum_n    E ( 2 (z_mj - x_nj)   / ls_j^2).

dk'/dr2 in closed form, finite at r = 0:  rbf -k'/2;  matern32 -(3/2) e^-a, a = sqrt(3 r2);  matern52 -(5/6)(1 + a) e^-a, a = sqrt(5 r2).

Every function returns (g, A): two dicts with the keys "ls" (d), "sf2" (scalar array) and "Z" (M x d).  A is the CONDITION SCALE of the
component: the same sum with every factor replaced by its absolute value -- (|Phibar| + |Phibar^T|) |K|, |bbar| |y|^T, |dK/dtheta| and
|kappabar| N.  A floating-point evaluation in any order is off by (chain length) x (unit round-off) x A at most; one missing (n, m) term is
~ A / (N M).  The comparison everywhere is component-wise  |got - ref| <= TAU * A  (``worst_ratio`` / ``assert_close``).
"""
import numpy as np

LD = np.longdouble
TAU = 1e-12
KID = {"rbf": 0, "matern32": 1, "matern52": 2, 0: 0, 1: 1, 2: 2}


def _ld(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64).astype(LD)


def _ls(ls, d):
    v = _ld(ls.tolist() if hasattr(ls, "tolist") else ls).reshape(-1)
    return np.repeat(v, d) if v.size == 1 and d > 1 else v


def profile(r2, kernel_id):
    """(k', dk'/dr2) of the unit-amplitude profile at the scaled squared distance r2 (long double)."""
    kid = KID[kernel_id]
    if kid == 0:
        k = np.exp(-r2 / 2)
        return k, -k / 2
    if kid == 1:
        a = np.sqrt(3 * r2)
        e = np.exp(-a)
        return (1 + a) * e, -(LD(3) / 2) * e
    a = np.sqrt(5 * r2)
    e = np.exp(-a)
    return (1 + a + a * a / 3) * e, -(LD(5) / 6) * (1 + a) * e


def _dot(a, b, to=""):
    """sum(a o b) over everything (to = "") or down to the columns (to = "m"): a long-double loop without the product as a temporary."""
    return np.einsum("nm,nm->" + to, a, b)


def _differences(rows_scaled, cols_scaled):
    """([D_j], [D_j^2], r2) with D_j[n][m] = (z_mj - x_nj) / ls_j, one n x M array per dimension."""
    D = [cols_scaled[None, :, j] - rows_scaled[:, j, None] for j in range(cols_scaled.shape[1])]
    W = [Dj * Dj for Dj in D]
    r2 = W[0].copy()
    for Wj in W[1:]:
        r2 += Wj
    return D, W, r2


def _contract(rows, cols, ls, sf2, S, Sabs, bbar, y, kernel_id, budget=1 << 18):
    """sum over the rows (in chunks) of everything pass 2 sums: (g, A) of the part through K, without the kappa term.
    rows: n x d (the data), cols: M x d (the inducing inputs), S = Phibar + Phibar^T, Sabs = |Phibar| + |Phibar^T|."""
    n_all, d = rows.shape
    M = cols.shape[0]
    cs = cols / ls
    g = {"ls": np.zeros(d, LD), "sf2": np.zeros((), LD), "Z": np.zeros((M, d), LD)}
    A = {"ls": np.zeros(d, LD), "sf2": np.zeros((), LD), "Z": np.zeros((M, d), LD)}
    step = max(1, budget // (M * d))
    for s in range(0, n_all, step):
        D, W, r2 = _differences(rows[s:s + step] / ls, cs)
        kp, hp = profile(r2, kernel_id)                                # n x M
        yc = y[s:s + step]
        Kbar = sf2 * (kp @ S) + yc[:, None] * bbar[None, :]            # S is symmetric: Kbar_uf^T, n x M
        Kbar_abs = sf2 * (kp @ Sabs) + np.abs(yc)[:, None] * np.abs(bbar)[None, :]
        g["sf2"] += _dot(Kbar, kp)
        A["sf2"] += _dot(Kbar_abs, kp)
        E, Eabs = Kbar * (sf2 * hp), Kbar_abs * (sf2 * np.abs(hp))     # dL/dr2 and its scale
        for j in range(d):
            g["ls"][j] += _dot(E, W[j])
            A["ls"][j] += _dot(Eabs, W[j])
            g["Z"][:, j] += _dot(E, D[j], "m")
            A["Z"][:, j] += _dot(Eabs, np.abs(D[j]), "m")
    for out in (g, A):
        out["ls"] = out["ls"] * (2 / ls)
        out["Z"] = out["Z"] * (2 / ls)[None, :]
    g["ls"] = -g["ls"]
    return g, A


def _bwd(X, y, Z, ls, sf2, P, Pabs, bbar, kappabar, kernel_id):
    X, y, Z, bbar = _ld(X), _ld(y).reshape(-1), _ld(Z), _ld(bbar).reshape(-1)
    N, d = X.shape
    sf2, kappabar = LD(float(sf2)), LD(float(kappabar))
    g, A = _contract(X, Z, _ls(ls, d), sf2, P + P.T, Pabs + Pabs.T, bbar, y, kernel_id)
    g["sf2"] = g["sf2"] + kappabar * N
    A["sf2"] = A["sf2"] + abs(kappabar) * N
    return g, A


def bwd_reference(X, y, Z, ls, sf2, Phibar, bbar, kappabar, kernel_id):
    """(g, A) of sgp_suffstats_bwd: the gradient of L above with respect to ls, sf2 and Z, and its condition scale."""
    P = _ld(Phibar)
    return _bwd(X, y, Z, ls, sf2, P, np.abs(P), bbar, kappabar, kernel_id)


def bwd_factored_reference(X, y, Z, ls, sf2, Linv, Cw, s2, bbar, kappabar, kernel_id):
    """(g, A) of sgp_suffstats_bwd_factored(_ex): the same with Phibar = L^-T (Cw / 2 s2) L^-1 formed in long double from the M x M
    ``Linv`` the caller read back from the device (the factorization is not under test); A takes |L^-T| |Cw / 2 s2| |L^-1| for |Phibar|."""
    Li, C = _ld(Linv), _ld(Cw) / (2 * LD(float(s2)))
    P = Li.T @ C @ Li
    Pabs = np.abs(Li).T @ np.abs(C) @ np.abs(Li)
    return _bwd(X, y, Z, ls, sf2, P, Pabs, bbar, kappabar, kernel_id)


def kuu_bwd_reference(Z, ls, sf2, Kuubar, kernel_id, budget=1 << 18):
    """(g, A) of sgp_kuu_bwd: the gradient of sum(Kuubar o K_uu(Z)) -- the diagonal (r = 0) included, a jitter has no gradient -- with
    respect to ls, sf2 and Z.  Row m and column m of K_uu both move with z_m: g_Z[m] sums (Kuubar + Kuubar^T)[m][m'] dK/dz_m."""
    Z, Kb = _ld(Z), _ld(Kuubar)
    M, d = Z.shape
    ls = _ls(ls, d)
    sf2 = LD(float(sf2))
    zs = Z / ls
    Kabs = np.abs(Kb)
    S, Sabs = Kb + Kb.T, Kabs + Kabs.T
    g = {"ls": np.zeros(d, LD), "sf2": np.zeros((), LD), "Z": np.zeros((M, d), LD)}
    A = {"ls": np.zeros(d, LD), "sf2": np.zeros((), LD), "Z": np.zeros((M, d), LD)}
    step = max(1, budget // (M * d))
    for s in range(0, M, step):
        # the chunk's rows m' of K_uu against every column m: D_j[m'][m] = (z_mj - z_m'j) / ls_j, sums "down to the columns" are g_Z[m]
        D, W, r2 = _differences(zs[s:s + step], zs)
        kp, hp = profile(r2, kernel_id)
        g["sf2"] += _dot(Kb[s:s + step], kp)
        A["sf2"] += _dot(Kabs[s:s + step], kp)
        h, habs = sf2 * hp, sf2 * np.abs(hp)
        E, Eabs = Kb[s:s + step] * h, Kabs[s:s + step] * habs
        Es, Esabs = S[s:s + step] * h, Sabs[s:s + step] * habs       # (S is symmetric: its rows are its columns)
        for j in range(d):
            g["ls"][j] += _dot(E, W[j])
            A["ls"][j] += _dot(Eabs, W[j])
            g["Z"][:, j] += _dot(Es, D[j], "m")
            A["Z"][:, j] += _dot(Esabs, np.abs(D[j]), "m")
    for out in (g, A):
        out["ls"] = out["ls"] * (2 / ls)
        out["Z"] = out["Z"] * (2 / ls)[None, :]
    g["ls"] = -g["ls"]
    return g, A


def pack(g, want_gz):
    """[g_ls | g_sf2 | g_Z (only with want_gz)] as one long-double vector: the layout of the engines' packed gradients."""
    parts = [g["ls"].reshape(-1), g["sf2"].reshape(1)] + ([g["Z"].reshape(-1)] if want_gz else [])
    return np.concatenate(parts)


def worst_ratio(got, ref, A, slack=None):
    """max over the components of |got - ref| / A (``slack``: an absolute allowance per component taken off the error first).
    A component whose A is 0 has no term at all: there anything but the exact value counts as infinitely wrong; NaN is infinitely wrong."""
    got, ref, A = _ld(got).reshape(-1), np.asarray(ref, LD).reshape(-1), np.asarray(A, LD).reshape(-1)
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    err = np.abs(got - ref)
    if slack is not None:
        err = np.maximum(err - np.asarray(slack, LD).reshape(-1), 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, LD(0), err / A)
    ratio = np.where(np.isnan(ratio), LD(np.inf), ratio)
    return float(ratio.max()) if ratio.size else 0.0


def assert_close(got, ref, A, tau=TAU, slack=None, what=""):
    """The one comparison of these tests; returns the worst err / A it saw."""
    w = worst_ratio(got, ref, A, slack)
    assert w <= tau, "%s: worst |got - ref| / A = %.3e > %.1e" % (what, w, tau)
    return w


def scalar_L(X, y, Z, ls, sf2, Phibar, bbar, kappabar, kernel_id):
    """The scalar L itself in long double (small shapes: the tests differentiate it numerically)."""
    X, y, Z, P, bbar = _ld(X), _ld(y).reshape(-1), _ld(Z), _ld(Phibar), _ld(bbar).reshape(-1)
    ls = _ls(ls, X.shape[1])
    D = Z[:, None, :] / ls - (X / ls)[None, :, :]
    K = LD(float(sf2)) * profile((D * D).sum(-1), kernel_id)[0]         # M x N
    return (P * (K @ K.T)).sum() + bbar @ (K @ y) + LD(float(kappabar)) * X.shape[0] * LD(float(sf2))


def scalar_Luu(Z, ls, sf2, Kuubar, kernel_id):
    """sum(Kuubar o K_uu(Z)) in long double."""
    Z = _ld(Z)
    ls = _ls(ls, Z.shape[1])
    D = Z[:, None, :] / ls - (Z / ls)[None, :, :]
    return (_ld(Kuubar) * (LD(float(sf2)) * profile((D * D).sum(-1), kernel_id)[0])).sum()
