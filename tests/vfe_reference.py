"""Long-double reference of the collapsed (VFE) bound and of its complete gradient, with the condition scale of every output.

TEST INFRASTRUCTURE ONLY -- numpy ``longdouble`` (x87 extended: eps 1.1e-19) on the host, the style of tests/pass2_reference.py.  It is the
yardstick the single launch sgp_small_eval (tests/test_small_reference_gpu.py) and the multi-launch forms of CollapsedBound are held against.

    K = k(Z, Z) + J I ,  L = chol(K) ,  A = L^-1 K_uf ,  B = I + A A^T / s2 ,  L_B = chol(B) ,  u = A y ,  c0 = L_B^-1 u ,  g = B^-1 u
    kappa = N k(x, x)

    F        = -[ N/2 log 2 pi + N/2 log s2 + sum log diag L_B + (yy / s2 - c0.c0 / s2^2) / 2 + (kappa - sum A o A) / (2 s2) ]
             =  logmarg - trace_term          (the first four terms, the last one)
    Kbar_uf  = L^-T [ (I - B^-1 - g g^T / s2^2) A + g y^T / s2 ] / s2
    Kbar_uu  = -1/2 L^-T (B + B^-1 - 2 I + g g^T / s2^2) L^-1
    g_theta  = sum Kbar_uf o dK_uf/dtheta + sum Kbar_uu o dK_uu/dtheta - N / (2 s2) dk(x, x)/dtheta      theta in ls_j, sf2, Z (or a block slot)
    g_s2     = -[ N / (2 s2) - (M - tr B^-1) / (2 s2) - yy / (2 s2^2) + u.g / s2^3 - g^T (A A^T) g / (2 s2^4) - (kappa - sum A o A) / (2 s2^2) ]

The jitter J has no gradient.  The rows are walked in chunks (``_contract``).

CONDITION SCALES.  Every output comes with the same sum in which every final factor is replaced by its absolute value, formed in the
WHITENED basis the kernel works in -- from the actual A, Kbar_uf and Kbar_uu:

    S_F      = N/2 log 2 pi + |N/2 log s2| + sum |log diag L_B| + (yy / s2 + c0.c0 / s2^2) / 2 + (kappa + sum A o A) / (2 s2)
    A_theta  = sum |Kbar_uf| o |dK_uf/dtheta| + sum |Kbar_uu| o |dK_uu/dtheta| + N / (2 s2) |dk(x, x)/dtheta|
    A_s2     = the six terms of g_s2 in absolute value, a difference inside a term (M - tr B^-1, kappa - sum A o A) counted as a sum

A scale built from |L^-1| |K_uf| or from Phibar = L^-T Wbar L^-1 would be cond(K_uu) too large and hide anything; this one is not.  The
comparison everywhere is component-wise  |got - ref| <= tol * scale.

``dtype=np.float64`` runs the same closed form in float64, in one of two orders: ``order="inverse"`` through the explicit L^-1 (row loops),
``order="substitution"`` with triangular solves only, as the kernel does (numpy.linalg.cholesky + scipy.linalg.solve_triangular).  In long
double the two coincide.  ``measure_e64`` is the worse of the two against the long-double value, per output group, in units of the scale.

``mutate`` breaks one thing at a time (MUTATIONS) so that a test can show the comparison failing on it.

Two thin layers: the NUTS target of mode 1 (priors, log transforms, chain rule; a component's scale is the scale of its natural gradient
times the Jacobian factor plus the absolute prior terms), and composite kernels through ``sgpmc_comp_reference.comp_k``.

The outputs are laid out as the kernel's:  out = [value | kernel hyper-parameter gradients (nh) | noise | logmarg | trace_term]  and g_Z.
"""
import functools

import numpy as np

import sgpmc_comp_reference as CR
from pass2_reference import KID, LD, kuu_bwd_reference, profile  # noqa: F401
from sgpmc_reference import chol_ld, tri_inv_ld

UNDERFLOW = LD(1e-290)  # the slack of exact_batch_reference: long double keeps terms that lie below the whole float64 range
MARGIN = 10
FLOOR = 1e-13
MUTATIONS = ("drop_row", "no_gg_kuu", "trace_pad", "kuu_z_once", "matern_h0", "matern_h_nan", "matern_h_rbf", "no_jitter")


def _pi(F):
    return np.arccos(F(-1))


def _profile(r2, kid, F, mutate=None):
    """(k', dk'/dr2) in the dtype F; long double goes through pass2_reference.profile."""
    kid = KID[kid]
    if F is LD:
        k, h = profile(r2, kid)
    elif kid == 0:
        k = np.exp(-r2 / 2)
        h = -k / 2
    elif kid == 1:
        a = np.sqrt(3 * r2)
        e = np.exp(-a)
        k, h = (1 + a) * e, -(F(3) / 2) * e
    else:
        a = np.sqrt(5 * r2)
        e = np.exp(-a)
        k, h = (1 + a + a * a / 3) * e, -(F(5) / 6) * (1 + a) * e
    if kid and mutate == "matern_h0":
        h = np.where(r2 == 0, F(0), h)
    if kid and mutate == "matern_h_nan":  # the slope taken as (dk/dr) / 2r without a guard: 0 / 0 at r = 0
        h = np.where(r2 == 0, F(np.nan), h)
    if kid and mutate == "matern_h_rbf":
        h = -k / 2
    return k, h


def _stationary_k(rows, cols, ls, sf2, kid, F):
    """sf2 k'(rows_i, cols_j): len(rows) x len(cols)."""
    rs, cs = rows / ls, cols / ls
    r2 = np.zeros((rows.shape[0], cols.shape[0]), F)
    for j in range(rows.shape[1]):
        dj = cs[None, :, j] - rs[:, j, None]
        r2 += dj * dj
    return sf2 * _profile(r2, kid, F)[0]


def _contract(rows, cols, ls, sf2, Kbar, kid, F, both=False, z_once=False, mutate=None, budget=1 << 18):
    """sum(Kbar o dK/dtheta) for K[n][m] = sf2 k'(rows_n, cols_m) and its scale, rows in chunks: (g, A) with the keys ls, sf2, Z.
    dK/dZ moves the columns; ``both``: rows and columns are the same inducing inputs (K_uu), so row m moves with z_m too and g_Z[m]
    sums (Kbar + Kbar^T)[.][m] (``z_once``: the deliberate defect that forgets it)."""
    n_all, d = rows.shape
    M = cols.shape[0]
    cs = cols / ls
    g = {"ls": np.zeros(d, F), "sf2": np.zeros((), F), "Z": np.zeros((M, d), F)}
    A = {"ls": np.zeros(d, F), "sf2": np.zeros((), F), "Z": np.zeros((M, d), F)}
    Kabs = np.abs(Kbar)
    Kz, Kzabs = (Kbar + Kbar.T, Kabs + Kabs.T) if both and not z_once else (Kbar, Kabs)
    step = max(1, budget // (M * d))
    for s in range(0, n_all, step):
        rs = rows[s:s + step] / ls
        D = [cs[None, :, j] - rs[:, j, None] for j in range(d)]
        W = [Dj * Dj for Dj in D]
        r2 = W[0].copy()
        for Wj in W[1:]:
            r2 += Wj
        kp, hp = _profile(r2, kid, F, mutate)
        Kb, Ka = Kbar[s:s + step], Kabs[s:s + step]
        g["sf2"] += np.einsum("nm,nm->", Kb, kp)
        A["sf2"] += np.einsum("nm,nm->", Ka, kp)
        h, habs = sf2 * hp, sf2 * np.abs(hp)
        E, Eabs, Ez, Ezabs = Kb * h, Ka * habs, Kz[s:s + step] * h, Kzabs[s:s + step] * habs
        for j in range(d):
            g["ls"][j] += np.einsum("nm,nm->", E, W[j])
            A["ls"][j] += np.einsum("nm,nm->", Eabs, W[j])
            g["Z"][:, j] += np.einsum("nm,nm->m", Ez, D[j])
            A["Z"][:, j] += np.einsum("nm,nm->m", Ezabs, np.abs(D[j]))
    for out in (g, A):
        out["ls"] = out["ls"] * (2 / ls)
        out["Z"] = out["Z"] * (2 / ls)[None, :]
    g["ls"] = -g["ls"]
    return g, A


def _core(K, Kuf, y, s2, kdiag, F, order, mutate):
    """Everything that does not depend on the kind of kernel: the values, their scales, Kbar_uf (M x N), Kbar_uu, g_s2."""
    M, N = Kuf.shape
    I = np.eye(M, dtype=F)
    if F is LD or order == "inverse":
        def factor(S):
            Lf = chol_ld(S, F)
            Lfi = tri_inv_ld(Lf, F)
            return Lf, (lambda R: Lfi @ R), (lambda R: Lfi.T @ R)
    else:
        from scipy.linalg import solve_triangular

        def factor(S):
            Lf = np.linalg.cholesky(S)
            return Lf, (lambda R: solve_triangular(Lf, R, lower=True)), (lambda R: solve_triangular(Lf.T, R, lower=False))
    _, fwdK, bwdK = factor(K)
    A = fwdK(Kuf)
    AAt = A @ A.T
    B = I + AAt / s2
    LB, fwdB, bwdB = factor(B)
    u = A @ y
    c0 = fwdB(u)
    g = bwdB(c0)
    Binv = bwdB(fwdB(I))
    yy, cc, sumA2, kappa = y @ y, c0 @ c0, (A * A).sum(), N * kdiag
    half, two = F(1) / 2, F(2)
    logs = np.log(np.diagonal(LB))
    lead = (F(N) / 2) * np.log(2 * _pi(F)), (F(N) / 2) * np.log(s2)
    logmarg = -(lead[0] + lead[1] + logs.sum() + half * (yy / s2 - cc / (s2 * s2)))
    S_logmarg = lead[0] + abs(lead[1]) + np.abs(logs).sum() + half * (yy / s2 + cc / (s2 * s2))
    trace = (kappa - sumA2) / (two * s2)
    S_trace = (kappa + sumA2) / (two * s2)
    gg = np.outer(g, g) / (s2 * s2)
    Abar = ((I - Binv - gg) @ A + np.outer(g, y) / s2) / s2
    if mutate == "drop_row":
        Abar[:, -1] = 0
    Kbar_uf = bwdK(Abar)
    C = B + Binv - two * I + (0 if mutate == "no_gg_kuu" else gg)
    Kbar_uu = -half * bwdK(bwdK(C).T).T
    trBinv = np.trace(Binv)
    count = F((64 if M <= 64 else 128) if mutate == "trace_pad" else M)
    Ag = A.T @ g
    s22 = s2 * s2
    t = [F(N) / (two * s2), -(count - trBinv) / (two * s2), -yy / (two * s22), (u @ g) / (s22 * s2), -(Ag @ Ag) / (two * s22 * s22),
         -(kappa - sumA2) / (two * s22)]
    A_s2 = (abs(t[0]) + (count + abs(trBinv)) / (two * s2) + abs(t[2]) + abs(t[3]) + abs(t[4]) + (kappa + sumA2) / (two * s22))
    return {"F": logmarg - trace, "S_F": S_logmarg + S_trace, "logmarg": logmarg, "S_logmarg": S_logmarg, "trace": trace, "S_trace": S_trace,
            "Kbar_uf": Kbar_uf, "Kbar_uu": Kbar_uu, "g_s2": -(t[0] + t[1] + t[2] + t[3] + t[4] + t[5]), "A_s2": A_s2, "A": A, "B": B}


def _c(a, F):
    """``a`` in the dtype F: through float64 (what the device is handed), unless it already is long double (the finite differences of
    tests/test_vfe_reference.py step their inputs in long double)."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return (a if a.dtype == LD else a.astype(np.float64)).astype(F)


def stationary(X, y, Z, ls, sf2, s2, jitter, kernel, dtype=LD, order="inverse", mutate=None, grads=True):
    """(ref, A): dicts with F, logmarg, trace, g_ls (d), g_sf2, g_s2, g_Z (M x d) -- A the condition scale of each."""
    assert mutate is None or mutate in MUTATIONS
    F = dtype
    X, y, Z = _c(X, F), _c(y, F).reshape(-1), _c(Z, F)
    N, d = X.shape
    M = Z.shape[0]
    ls = _c(ls, F).reshape(-1)
    ls = np.repeat(ls, d) if ls.size == 1 and d > 1 else ls
    sf2, s2, J = F(_c(sf2, F)), F(_c(s2, F)), F(_c(jitter, F))
    K = _stationary_k(Z, Z, ls, sf2, kernel, F) + (0 if mutate == "no_jitter" else J) * np.eye(M, dtype=F)
    Kuf = _stationary_k(Z, X, ls, sf2, kernel, F)
    c = _core(K, Kuf, y, s2, sf2, F, order, mutate)
    ref = {"F": c["F"], "logmarg": c["logmarg"], "trace": c["trace"], "g_s2": c["g_s2"]}
    A = {"F": c["S_F"], "logmarg": c["S_logmarg"], "trace": c["S_trace"], "g_s2": c["A_s2"]}
    if grads:
        gf, af = _contract(X, Z, ls, sf2, c["Kbar_uf"].T, kernel, F, mutate=mutate)
        gu, au = _contract(Z, Z, ls, sf2, c["Kbar_uu"], kernel, F, both=True, z_once=mutate == "kuu_z_once", mutate=mutate)
        k2 = F(N) / (2 * s2)
        ref.update(g_ls=gf["ls"] + gu["ls"], g_sf2=gf["sf2"] + gu["sf2"] - k2, g_Z=gf["Z"] + gu["Z"])
        A.update(g_ls=af["ls"] + au["ls"], g_sf2=af["sf2"] + au["sf2"] + k2, g_Z=af["Z"] + au["Z"])
        ref["Kbar_uu"] = c["Kbar_uu"]
    return ref, A


def stationary_nuts(X, y, Z, theta, jitter, kernel, dtype=LD, order="inverse", mutate=None):
    """The NUTS target of mode 1 at theta = [log ls_1..d | log sig_f | log sig_n]: ls ~ Gamma(2, 1), sig_f, sig_n ~ HalfCauchy(1), log
    transforms.  (ref, A) with F (the log density), g_ls, g_sf2, g_s2 (now d / d theta), logmarg, trace."""
    F = dtype
    th = _c(theta, F).reshape(-1)
    d = th.size - 2
    ls, sf, sn = np.exp(th[:d]), np.exp(th[d]), np.exp(th[d + 1])
    r, a = stationary(X, y, Z, ls, sf * sf, sn * sn, jitter, kernel, F, order, mutate)
    c = np.log(F(2)) - np.log(_pi(F))
    ref = {"logmarg": r["logmarg"], "trace": r["trace"]}
    A = {"logmarg": a["logmarg"], "trace": a["trace"]}
    ref["F"] = r["F"] + (np.log(ls) - ls).sum() + 2 * c - np.log1p(sf * sf) - np.log1p(sn * sn) + th.sum()
    A["F"] = a["F"] + (np.abs(np.log(ls)) + ls).sum() + 2 * abs(c) + np.log1p(sf * sf) + np.log1p(sn * sn) + np.abs(th).sum()
    ref["g_ls"] = ls * r["g_ls"] + 1 - ls + 1
    A["g_ls"] = ls * a["g_ls"] + 1 + ls + 1
    for key, s in (("g_sf2", sf), ("g_s2", sn)):
        ref[key] = 2 * s * s * r[key] - 2 * s * s / (1 + s * s) + 1
        A[key] = 2 * s * s * a[key] + 2 * s * s / (1 + s * s) + 1
    return ref, A


def composite(X, y, Z, block, s2, jitter, dtype=LD, order="inverse", mutate=None):
    """(ref, A) for a composite kernel (the parameter block of include/sgp.h): F, logmarg, trace, g_block (all COMP_LEN slots, zero
    where a slot carries no derivative), g_s2.  No dF/dZ: the single launch has none for composite kernels."""
    F = dtype
    X, y, Z = _c(X, F), _c(y, F).reshape(-1), _c(Z, F)
    blk = _c(block, F).reshape(-1)
    s2, J = F(_c(s2, F)), F(_c(jitter, F))
    N, M = X.shape[0], Z.shape[0]
    b64 = np.asarray(blk, np.float64)
    amps = CR.amp_slots(b64)
    Kuu, dKuu = CR.comp_k(Z, Z, blk, F, True)
    Kuf, dKuf = CR.comp_k(Z, X, blk, F, True)
    K = Kuu + (0 if mutate == "no_jitter" else J) * np.eye(M, dtype=F)
    c = _core(K, Kuf, y, s2, sum(blk[a] for a in amps), F, order, mutate)
    ref = {"F": c["F"], "logmarg": c["logmarg"], "trace": c["trace"], "g_s2": c["g_s2"], "g_block": np.zeros(CR.COMP_LEN, F)}
    A = {"F": c["S_F"], "logmarg": c["S_logmarg"], "trace": c["S_trace"], "g_s2": c["A_s2"], "g_block": np.zeros(CR.COMP_LEN, F)}
    Kf, Ku = c["Kbar_uf"], c["Kbar_uu"]
    for s in CR.param_slots(b64):
        k2 = F(N) / (2 * s2) if s in amps else F(0)
        ref["g_block"][s] = np.einsum("ij,ij->", Kf, dKuf[s]) + np.einsum("ij,ij->", Ku, dKuu[s]) - k2
        A["g_block"][s] = np.einsum("ij,ij->", np.abs(Kf), np.abs(dKuf[s])) + np.einsum("ij,ij->", np.abs(Ku), np.abs(dKuu[s])) + k2
    return ref, A


def composite_nuts(X, y, Z, structure, free, theta, jitter, dtype=LD, order="inverse", mutate=None):
    """The composite NUTS target of mode 1: theta = [log of every free parameter | log sigma], ``free`` = [(slot, role, prior sd)] with
    role 0 an amplitude sd (amp2 = v^2), 1 a lengthscale, 2 an aux value; log-parameters ~ Normal(0, sd) sampled in log space,
    sigma ~ HalfNormal(1) log-transformed.  (ref, A) with F, g_free (len(free)), g_s2, logmarg, trace."""
    F = dtype
    th = _c(theta, F).reshape(-1)
    blk = _c(structure, F).reshape(-1).copy()
    v = np.exp(th[:-1])
    for k, (slot, role, _) in enumerate(free):
        blk[slot] = v[k] * v[k] if role == 0 else v[k]
    tn = th[-1]
    sig2 = np.exp(tn) ** 2
    r, a = composite(X, y, Z, blk, sig2, jitter, F, order, mutate)
    ref = {"logmarg": r["logmarg"], "trace": r["trace"], "g_free": np.zeros(len(free), F)}
    A = {"logmarg": a["logmarg"], "trace": a["trace"], "g_free": np.zeros(len(free), F)}
    lp, alp = r["F"], a["F"]
    halflog2pi = np.log(2 * _pi(F)) / 2
    for k, (slot, role, sd) in enumerate(free):
        sd, t = F(sd), th[k]
        lp = lp - (t / sd) ** 2 / 2 - np.log(sd) - halflog2pi
        alp = alp + (t / sd) ** 2 / 2 + abs(np.log(sd)) + halflog2pi
        jac = 2 * v[k] * v[k] if role == 0 else v[k]
        ref["g_free"][k] = jac * r["g_block"][slot] - t / (sd * sd)
        A["g_free"][k] = jac * a["g_block"][slot] + abs(t) / (sd * sd)
    c = np.log(2 / _pi(F)) / 2
    ref["F"] = lp + c - sig2 / 2 + tn
    A["F"] = alp + abs(c) + sig2 / 2 + abs(tn)
    ref["g_s2"] = 2 * sig2 * r["g_s2"] - sig2 + 1
    A["g_s2"] = 2 * sig2 * a["g_s2"] + sig2 + 1
    return ref, A


# ---------------------------------------------------------------------------------------------------------------------------------
# the cells: the smallest shapes that reach each branch of the single launch
# ---------------------------------------------------------------------------------------------------------------------------------
def _cell(N, M, d, kernel, sharp=False, tag="", **kw):
    c = {"N": N, "M": M, "d": d, "kernel": kernel, "sharp": sharp, "sf2": 1.3, "s2": 0.07, "jitter": 1e-6, "seed": 1000 * N + 10 * M + d,
         "ls": [1.0 + 0.1 * j for j in range(d)], "mode": 0, "want_gz": kernel != "composite", "near": False, "budget": 0}
    c.update(kw)
    name = "-".join(str(v) for v in (N, M, d, kernel)) + ("-" + tag if tag else "")
    return name, c


def _two_factor_block():
    from oracle import composite_oracle as CO
    return CO.make_block([(1.3, [(CO.MATERN52, 3.0), (CO.RATQUAD, 4.0, 2.0)])])


def _co2():
    from oracle import composite_oracle as CO
    return CO.co2_block()


LS24 = [5.0 * (1.0 + 0.1 * j) for j in range(24)]
LS2 = [0.4, 0.44]  # rbf with M >= 60 inducing inputs in two dimensions: short enough for the sharpness condition of the CPU tests
SHARP = [
    _cell(1, 1, 1, "rbf", True), _cell(63, 15, 2, "rbf", True, seed=63153), _cell(64, 16, 2, "matern32", True),
    _cell(65, 17, 2, "rbf", True), _cell(129, 48, 3, "matern52", True), _cell(130, 49, 1, "rbf", True, ls=[0.05], seed=130492),
    _cell(200, 63, 2, "rbf", True, ls=LS2), _cell(200, 64, 2, "matern32", True), _cell(200, 65, 2, "rbf", True, ls=LS2, seed=200655),
    _cell(130, 127, 2, "matern52", True, ls=LS2, seed=131273), _cell(130, 128, 3, "rbf", True, ls=[0.6, 0.66, 0.72]),
    _cell(64, 16, 24, "matern32", True, ls=LS24), _cell(40, 60, 2, "rbf", True, ls=LS2, seed=40604),
]
REDUCTION = [_cell(1984, 17, 2, "rbf"), _cell(1985, 17, 2, "rbf"), _cell(1920, 65, 2, "rbf"), _cell(1921, 65, 2, "rbf"),
             _cell(2049, 128, 3, "rbf"), _cell(13313, 20, 2, "rbf")]
BUDGET = [_cell(449, M, 2, "rbf", tag="cu%d" % b, budget=b) for b in (4, 6) for M in (17, 65)]
ILL = [
    _cell(200, 64, 2, "rbf", tag="ill", ls=[3.0, 3.0], s2=1e-3), _cell(300, 128, 1, "rbf", tag="ill", ls=[2.0], s2=1e-3),
    _cell(200, 33, 2, "matern32", tag="near", s2=1e-2, near=True), _cell(129, 65, 1, "rbf", tag="ls0.6", ls=[0.6]),
    _cell(200, 64, 2, "rbf", tag="sf100", sf2=100.0, s2=10.0),
]
NUTS = [_cell(65, 17, 2, "rbf", tag="nuts", mode=1, want_gz=False), _cell(200, 65, 2, "rbf", tag="nuts", mode=1, want_gz=False, ls=LS2, seed=200655),
        _cell(64, 16, 24, "matern32", tag="nuts", mode=1, want_gz=False, ls=LS24)]
COMPOSITE = [_cell(N, M, 1, "composite", tag="co2-mode%d" % mode, mode=mode, block="co2")
             for N, M in ((130, 17), (130, 64), (200, 65), (200, 128)) for mode in (0, 1)]
COMPOSITE += [_cell(65, 17, 8, "composite", tag="two-mode%d" % mode, mode=mode, block="two") for mode in (0, 1)]
# four theta rows of one small_eval_batch: the hyper-parameters of 200-65-2-rbf times 1, 1.1, 1.2, 1.3
BATCH = [_cell(200, 65, 2, "rbf", tag="batch%d" % k, seed=200655, ls=[v * (1 + 0.1 * k) for v in LS2], sf2=1.3 * (1 + 0.1 * k),
               s2=0.07 * (1 + 0.1 * k)) for k in range(4)]
CELLS = dict(SHARP + REDUCTION + BUDGET + ILL + NUTS + COMPOSITE + BATCH)
MULTI = dict([(n, c) for n, c in SHARP if c["M"] <= 65] + [_cell(130, 130, 2, "rbf")])  # the multi-launch forms (item 4)


def _spec(name):
    return CELLS[name] if name in CELLS else MULTI[name]


@functools.lru_cache(maxsize=None)
def cell_inputs(name):
    """The cell's inputs as float64 arrays: X standard normal, y = sin(sum X / sqrt d) + 0.1 noise, Z a random subset of X (so r = 0
    occurs; M > N: standard normal), theta as the entry point takes it."""
    c = _spec(name)
    N, M, d = c["N"], c["M"], c["d"]
    rs = np.random.RandomState(c["seed"])
    X = rs.standard_normal((N, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rs.standard_normal(N)
    Z = X[rs.permutation(N)[:M]].copy() if M <= N else rs.standard_normal((M, d))
    if c["near"]:  # every second row within 1e-4 of its neighbour
        Z[1::2] = Z[0:2 * (M // 2):2] + 1e-4 * rs.standard_normal((M // 2, d))
    inp = {"X": X, "y": y, "Z": Z, "jitter": c["jitter"], "kernel": c["kernel"], "mode": c["mode"], "want_gz": c["want_gz"]}
    if c["kernel"] == "composite":
        blk = np.asarray(_co2() if c["block"] == "co2" else _two_factor_block(), np.float64)
        inp["structure"] = blk
        if c["mode"] == 0:
            inp["theta"] = np.concatenate([blk, [c["s2"]]])
        else:
            amps = CR.amp_slots(blk)
            free = [(s, 0 if s in amps else (1 if (s - 1) % 8 in (3, 6) else 2), 1.0 if s in amps else 2.0) for s in CR.param_slots(blk)]
            inp["free"] = free
            nat = np.array([np.sqrt(blk[s]) if r == 0 else blk[s] for s, r, _ in free] + [np.sqrt(c["s2"])])
            inp["theta"] = np.log(nat) + 0.1 * rs.standard_normal(nat.size)
    elif c["mode"] == 0:
        inp["theta"] = np.array(list(c["ls"]) + [c["sf2"], c["s2"]])
    else:
        inp["theta"] = np.log(np.array(list(c["ls"]) + [np.sqrt(c["sf2"]), np.sqrt(c["s2"])])) + 0.1 * rs.standard_normal(d + 2)
    return inp


GROUPS = {"stationary": ("F", "g_ls", "g_sf2", "g_s2", "logmarg", "trace"), "composite0": ("F", "g_block", "g_s2", "logmarg", "trace"),
          "composite1": ("F", "g_free", "g_s2", "logmarg", "trace")}


def groups_of(name):
    c = _spec(name)
    g = GROUPS["stationary"] if c["kernel"] != "composite" else GROUPS["composite%d" % c["mode"]]
    return g + (("g_Z",) if c["want_gz"] else ())


def evaluate(name, dtype=LD, order="inverse", mutate=None):
    inp = cell_inputs(name)
    th = inp["theta"]
    X, y, Z, J = inp["X"], inp["y"], inp["Z"], inp["jitter"]
    if inp["kernel"] == "composite":
        if inp["mode"] == 0:
            return composite(X, y, Z, th[:-1], th[-1], J, dtype, order, mutate)
        return composite_nuts(X, y, Z, inp["structure"], inp["free"], th, J, dtype, order, mutate)
    if inp["mode"] == 0:
        return stationary(X, y, Z, th[:-2], th[-2], th[-1], J, inp["kernel"], dtype, order, mutate)
    return stationary_nuts(X, y, Z, th, J, inp["kernel"], dtype, order, mutate)


@functools.lru_cache(maxsize=None)
def cell_reference(name):
    """(ref, A) of the cell in long double; computed once per process and never changed (the arrays are read-only)."""
    ref, A = evaluate(name)
    for dct in (ref, A):
        for v in dct.values():
            if isinstance(v, np.ndarray) and v.ndim:
                v.setflags(write=False)
    return ref, A


def worst(got, ref, A, keys):
    """{key: worst |got - ref| / A over the key's components}, got in any dtype (UNDERFLOW is the only allowance)."""
    out = {}
    for k in keys:
        g, r, a = (np.asarray(x, LD).reshape(-1) for x in (got[k], ref[k], A[k]))
        assert g.shape == r.shape == a.shape, (k, g.shape, r.shape, a.shape)
        err = np.maximum(np.abs(g - r) - UNDERFLOW, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, LD(0), err / a)
        out[k] = float(np.where(np.isnan(q), LD(np.inf), q).max())
    return out


def measure_e64(name):
    """{group: worst |float64 - long double| / scale}, the larger of the two float64 orders."""
    ref, A = cell_reference(name)
    keys = groups_of(name)
    e = {k: 0.0 for k in keys}
    for order in ("inverse", "substitution"):
        w = worst(evaluate(name, np.float64, order)[0], ref, A, keys)
        e = {k: max(e[k], w[k]) for k in keys}
    return e


STREAM_KEYS = ("F", "g_ls", "g_sf2", "g_s2", "g_Z")


def streaming64(name):
    """The STREAMING order in float64, as the device runs it (sgp_suffstats_fwd + sgp_bound_from_stats + pass 2): the unwhitened
    Phi = K_uf K_fu and b = K_uf y, W = L^-1 Phi L^-T in the tail, the adjoints in the whitened sandwich L^-T [C | S] L^-1
    (oracle.bound_from_stats(whitened=True): the textbook Kuu^-1 - Sigma^-1 - ... form is NOT what the library evaluates, its
    cond(K_uu)-sized cancellations would inflate the gradients' level by 10 to 10^9), then Kbar_uf = 2 Phibar K_uf + bbar y^T
    contracted with dK.  This is oracle.grads_analytic(whitened=True) with the contraction of this module."""
    import torch
    from oracle import vfe_oracle as O
    inp, c = cell_inputs(name), _spec(name)
    th = inp["theta"]
    X, y, Z, ls, sf2, s2 = inp["X"], inp["y"], inp["Z"], th[:-2], float(th[-2]), float(th[-1])
    N, kid, F = X.shape[0], KID[c["kernel"]], np.float64
    Kuf = _stationary_k(Z, X, ls, F(sf2), kid, F)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)  # noqa: E731
    st = O.SuffStats(T(Kuf @ Kuf.T), T(Kuf @ y), float(y @ y), sf2 * N, N)
    r = O.bound_from_stats(O.kuu(T(Z), T(ls), sf2, inp["jitter"], kid), st, s2, with_adjoints=True, whitened=True)
    Kbar_uf = 2.0 * r["Phibar"].numpy() @ Kuf + np.outer(r["bbar"].numpy(), y)
    gf, _ = _contract(X, Z, ls, F(sf2), Kbar_uf.T, kid, F)
    gu, _ = _contract(Z, Z, ls, F(sf2), r["Kuubar"].numpy(), kid, F, both=True)
    return {"F": r["F"], "g_ls": gf["ls"] + gu["ls"], "g_sf2": gf["sf2"] + gu["sf2"] - N / (2 * s2), "g_s2": r["s2bar"], "g_Z": gf["Z"] + gu["Z"]}


def measure_e64_streaming(name):
    """{group: worst |float64 - long double| / scale} of the streaming order: ``streaming64`` against the long-double reference."""
    return worst(streaming64(name), *cell_reference(name), STREAM_KEYS)


def unpack(name, out, gz=None):
    """The device's out vector (and g_Z) as the reference's keys."""
    c = _spec(name)
    o = np.asarray(out, np.float64).reshape(-1)
    if c["kernel"] != "composite":
        d = c["d"]
        got = {"F": o[0], "g_ls": o[1:1 + d], "g_sf2": o[1 + d], "g_s2": o[2 + d], "logmarg": o[3 + d], "trace": o[4 + d]}
    else:
        nh = CR.COMP_LEN if c["mode"] == 0 else len(cell_inputs(name)["free"])
        got = {"F": o[0], ("g_block" if c["mode"] == 0 else "g_free"): o[1:1 + nh], "g_s2": o[1 + nh], "logmarg": o[2 + nh], "trace": o[3 + nh]}
    if gz is not None:
        got["g_Z"] = np.asarray(gz, np.float64)
    return got


def tolerance(e64):
    return MARGIN * max(e64, FLOOR)
