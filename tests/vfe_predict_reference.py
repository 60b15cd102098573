"""Long-double reference of the collapsed (VFE) sparse-GP predictive (mean and marginal variance per test point), with the condition
scale of both.

TEST INFRASTRUCTURE ONLY -- numpy ``longdouble`` on the host, built from tests/vfe_reference.py (``_stationary_k``, ``chol_ld``,
``tri_inv_ld``).  It is the yardstick sgp_vfe_predict_batch (tests/test_vfe_predict_gpu.py) and the CPU double
(tests/vfe_predict_double.py) are held against.

    K = sf2 k'(Z, Z) + J I ,  L = chol K ,  A = L^-1 K_uf ,  B = I + A A^T / s2 ,  L_B = chol B ,  u = A y ,  g = B^-1 u
    a*_t = L^-1 k_u*(t) ,  v_t = L_B^-1 a*_t ,  mean_t = a*_t^T g / s2 ,  var_t = sf2 - sum_m a*_mt^2 + sum_m v_mt^2  (+ s2)

Condition scales, formed in the WHITENED basis the kernel works in (the same sums with every final factor in absolute value):

    S_mu = sum_m |a*_m| |g_m| / s2 ,   S_v = sf2 + sum a*^2 + sum v^2  (+ s2)

The comparison is component-wise |got - ref| <= tol * S with ``vfe_reference.UNDERFLOW`` as the only allowance (at the far test point
k_u* underflows in float64 but not in long double), tol = ``vfe_reference.tolerance(e64)`` = 10 max(e64, 1e-13), e64 the worse of the two
float64 orders ("inverse": the explicit L^-1 and L_B^-1; "substitution": triangular solves) against long double over the cell's test
points, per output -- the rule of this kernel family.

``full_cov`` adds the covariance cov = K** - A*^T A* + C*^T C* (+ s2 I), A* = [a*_t], C* = [v_t], with the scale
S_cov = |K**| + |A*|^T |A*| + |C*|^T |C*| (+ s2 I), whose diagonal is var / S_v; ``predictive_composite`` is the same for a composite
kernel's parameter block.  The second half of this file holds the STREAMING predictive (sgp_predict from CollapsedBound's factors,
sgp_mixture_predict, sgp_mixture_predict_zs) to these: its cells, draws and float64 levels (tests/test_stream_predict.py).

``mutate`` breaks one thing at a time (MUTATIONS, COV_MUTATIONS) so that a test can show the comparison failing on it.

The cells are those of ``vfe_batch_double.CELLS`` with N <= 3000; a cell's test points are T = TN + 3 rows (TN the tile of the cell's
size class: two tiles, the last of three points): 1.5 x standard normal, row 0 the training row X[0], row 1 the inducing input Z[0], row 2
Z[-1] + 1e-9, row 3 the point 100 * 1 (mean exactly 0, var = sf2 (+ s2)).
"""
import functools

import numpy as np

import sgpmc_comp_reference as CR
import vfe_batch_double as VB
import vfe_reference as V
from vfe_reference import LD, UNDERFLOW, chol_ld, tolerance, tri_inv_ld  # noqa: F401

MUTATIONS = ("no_v2", "no_jitter", "no_noise")
COV_MUTATIONS = ("cov_no_ctc", "cov_noise_everywhere", "cov_kss_diag", "cov_row_shift", "mean_wrong_s2")  # (the streaming predictive's)
CELLS = [n for n in VB.CELLS if VB.spec(n)["N"] <= 3000]
TAGGED = ("200-64-2-rbf-ill", "200-33-2-matern32-near", "200-64-2-rbf-sf100")
KEYS = ("mean", "var")
COV_KEYS = ("mean", "var", "cov")   # with ``full_cov``
CAP_UNTAGGED, CAP_TAGGED = 1e-10, 1e-8  # what tol may reach at a cell (tests/test_vfe_predict.py): the rule cannot hide a failure
CAP_STREAMING = 1e-7                    # ... of the route through unwhitened statistics (untagged cells only: STREAM_CELLS below)


def tile_rows(M):
    """vb_tile_rows of M's size class (csrc/sgp_vfe_batch.hpp): 128 / 64 / 32 test points per tile."""
    return 2048 // (16 if M <= 16 else 32 if M <= 32 else 64)


def predictive(X, y, Z, Xs, ls, sf2, s2, jitter, kernel, pred_noise=True, dtype=LD, order="inverse", mutate=None, full_cov=False):
    """(ref, S): dicts with mean [T], var [T] (``full_cov``: and cov [T, T]) in ``dtype`` -- S the condition scale of each."""
    F = dtype
    X, Z, Xs = V._c(X, F), V._c(Z, F), V._c(Xs, F)
    d = X.shape[1]
    ls = V._c(ls, F).reshape(-1)
    ls = np.repeat(ls, d) if ls.size == 1 and d > 1 else ls
    sf2 = F(V._c(sf2, F))
    k = lambda rows, cols: V._stationary_k(rows, cols, ls, sf2, kernel, F)  # noqa: E731
    return _predictive(k, sf2, X, y, Z, Xs, s2, jitter, pred_noise, F, order, mutate, full_cov)


def predictive_composite(X, y, Z, Xs, block, s2, jitter, pred_noise=True, dtype=LD, order="inverse", mutate=None, full_cov=False):
    """``predictive`` for a composite kernel (the parameter block of include/sgp.h, through ``sgpmc_comp_reference.comp_k``); the prior
    variance k(x, x) is the sum of the block's amplitudes, as sgp_predict takes it."""
    F = dtype
    X, Z, Xs, blk = V._c(X, F), V._c(Z, F), V._c(Xs, F), V._c(block, F).reshape(-1)
    kdiag = sum(blk[a] for a in CR.amp_slots(np.asarray(blk, np.float64)))
    return _predictive(lambda rows, cols: CR.comp_k(rows, cols, blk, F), kdiag, X, y, Z, Xs, s2, jitter, pred_noise, F, order, mutate, full_cov)


def last_tile(T):
    """The columns of the last 64-column tile of T test points (the tile of the streaming predictive's column kernels)."""
    return np.arange(64 * ((T - 1) // 64), T)


def _predictive(k, kdiag, X, y, Z, Xs, s2, jitter, pred_noise, F, order, mutate, full_cov):
    """The closed form behind ``predictive`` / ``predictive_composite``: ``k(rows, cols)`` the kernel matrix in the dtype F (inputs
    already in F), ``kdiag`` = k(x, x)."""
    assert mutate is None or mutate in MUTATIONS + COV_MUTATIONS
    y = V._c(y, F).reshape(-1)
    M = Z.shape[0]
    sf2, s2, J = kdiag, F(V._c(s2, F)), F(V._c(jitter, F))
    K = k(Z, Z) + (0 if mutate == "no_jitter" else J) * np.eye(M, dtype=F)
    Kuf = k(Z, X)
    Kus = k(Z, Xs)
    I = np.eye(M, dtype=F)
    if F is LD or order == "inverse":
        def factor(S):
            Li = tri_inv_ld(chol_ld(S, F), F)
            return (lambda R: Li @ R), (lambda R: Li.T @ R)
    else:
        from scipy.linalg import solve_triangular

        def factor(S):
            Lf = np.linalg.cholesky(S)
            return (lambda R: solve_triangular(Lf, R, lower=True)), (lambda R: solve_triangular(Lf.T, R, lower=False))
    fwdK, _ = factor(K)
    A = fwdK(Kuf)
    fwdB, bwdB = factor(I + (A @ A.T) / s2)
    g = bwdB(fwdB(A @ y))
    a = fwdK(Kus)                       # M x T
    if mutate == "cov_row_shift":       # the last tile's points take their A* from the point before
        t = last_tile(a.shape[1])
        t = t[t > 0]
        a = a.copy()
        a[:, t] = fwdK(Kus)[:, t - 1]
    v = fwdB(a)
    noise = s2 if pred_noise and mutate != "no_noise" else F(0)
    a2, v2 = (a * a).sum(0), (F(0) * a[0] if mutate == "no_v2" else (v * v).sum(0))
    ref = {"mean": (a * g[:, None]).sum(0) / (s2 + J if mutate == "mean_wrong_s2" else s2), "var": sf2 - a2 + v2 + noise}
    S = {"mean": (np.abs(a) * np.abs(g)[:, None]).sum(0) / s2, "var": sf2 + a2 + (v * v).sum(0) + (s2 if pred_noise else F(0))}
    if full_cov:
        T = a.shape[1]
        Kss, eye = k(Xs, Xs), np.eye(T, dtype=F)
        prior = Kss * eye if mutate == "cov_kss_diag" else Kss
        ref["cov"] = prior - a.T @ a + (0 if mutate == "cov_no_ctc" else v.T @ v) + noise * (1 if mutate == "cov_noise_everywhere" else eye)
        S["cov"] = np.abs(Kss) + np.abs(a).T @ np.abs(a) + np.abs(v).T @ np.abs(v) + (s2 if pred_noise else F(0)) * eye
    return ref, S


@functools.lru_cache(maxsize=None)
def cell_points(name, T=None):
    """The cell's test points (float64, read-only): T = TN + 3 of them unless ``T`` says otherwise (the T-edge tests; the leading rows
    do not depend on T)."""
    inp, c = VB.inputs(name), VB.spec(name)
    d, T = c["d"], tile_rows(c["M"]) + 3 if T is None else T
    rs = np.random.RandomState(c["seed"] + 1)  # (a stream of its own beside the cell's; CAP_* hold what it gives)
    Xs = 1.5 * rs.standard_normal((max(T, 4), d))
    Xs[0], Xs[1], Xs[2], Xs[3] = inp["X"][0], inp["Z"][0], inp["Z"][-1] + 1e-9, 100.0
    Xs = Xs[:T].copy()
    Xs.setflags(write=False)
    return Xs


def evaluate(name, pred_noise=True, dtype=LD, order="inverse", mutate=None, T=None):
    inp = VB.inputs(name)
    th = inp["theta"]
    return predictive(inp["X"], inp["y"], inp["Z"], cell_points(name, T), th[:-2], th[-2], th[-1], inp["jitter"], inp["kernel"],
                      pred_noise, dtype, order, mutate)


@functools.lru_cache(maxsize=None)
def reference(name, pred_noise=True, T=None):
    """(ref, S) of the cell at its test points in long double; computed once per process and never changed."""
    ref, S = evaluate(name, pred_noise, T=T)
    for dct in (ref, S):
        for v in dct.values():
            v.setflags(write=False)
    return ref, S


def worst(got, ref, S, keys=KEYS):
    """{mean, var: worst |got - ref| / S over the test points}, UNDERFLOW the only allowance (``vfe_reference.worst``)."""
    return V.worst(got, ref, S, keys)


@functools.lru_cache(maxsize=None)
def measure_e64(name, pred_noise=True, T=None):
    """{mean, var: worst |float64 - long double| / scale over the cell's test points}, the larger of the two float64 orders."""
    ref, S = reference(name, pred_noise, T)
    e = {k: 0.0 for k in KEYS}
    for order in ("inverse", "substitution"):
        w = worst(evaluate(name, pred_noise, np.float64, order, T=T)[0], ref, S)
        e = {k: max(e[k], w[k]) for k in KEYS}
    return e


def tolerances(name, pred_noise=True, T=None):
    """{mean, var: vfe_reference.tolerance(e64)} of the cell."""
    return {k: tolerance(v) for k, v in measure_e64(name, pred_noise, T).items()}


def assert_close(got, name, pred_noise=True, what="", T=None, rows=None):
    """got: dict(mean, var) at the cell's test points (``rows``: the leading rows of them only).  Returns the worst ratios to the
    tolerance."""
    ref, S = reference(name, pred_noise, T)
    if rows is not None:
        ref, S = ({k: v[:rows] for k, v in dct.items()} for dct in (ref, S))
    w, tol = worst(got, ref, S), tolerances(name, pred_noise, T)
    for k in KEYS:
        assert w[k] <= tol[k], "%s %s: worst |%s - ref| / S = %.3e > tol %.3e" % (name, what, k, w[k], tol[k])
    return {k: w[k] / tol[k] for k in KEYS}


# ---------------------------------------------------------------------------------------------------------------------------------
# The STREAMING predictive -- what the large-M path hands its users: sgp_predict from the ``factors`` of CollapsedBound (either form),
# sgp_mixture_predict and sgp_mixture_predict_zs (tests/test_stream_predict.py on the CPU, tests/test_stream_predict_gpu.py).
#
# The cells are the smallest shapes that reach each branch of those kernels (named N-M-d-kernel[-tag], ``T`` test points): data and
# hyper-parameters by the recipe of ``vfe_reference.cell_inputs`` (sf2 1.3, s2 0.07, jitter 1e-6), test points by ``cell_points``'s.
# Draw k of a cell is theta_k = theta (1 + 0.05 k) -- nine of them make two batches of sgp_mixture_predict -- and, for the per-sample
# inducing inputs, Z_k = Z + 0.01 k noise_k.  Every draw is judged against the reference at its own theta_k and Z_k.
#
# Two float64 levels.  The WHITENED routes (CollapsedBound(form="whitened"), the mixture kernels: A = L^-1 K_uf is formed) are measured
# by the two orders of ``predictive``.  The STREAMING form goes through the unwhitened Phi = K_uf K_fu and loses cond(K_uu) eps there:
# its level is the worse of (a) oracle.vfe_oracle.predict as it is (triangular solves) and (b) the same with the explicit L^-1 sandwich
# W = L^-1 Phi L^-T and the explicit L_B^-1, which is how sgp_bound_from_stats hands ``factors`` to sgp_predict.  The streaming form is
# not run at the cells tagged ``ill``: its loss there is known, and is what the guarded walk of core.py exists for.
# ---------------------------------------------------------------------------------------------------------------------------------
def _scell(N, M, d, kernel, T, **kw):
    name, c = V._cell(N, M, d, kernel, **kw)
    c["T"] = T
    return name, c


LS3 = [0.6, 0.66, 0.72]
STREAM_CELLS = dict([
    _scell(1, 1, 1, "rbf", 5),                                # M = N = 1, T < 64
    _scell(50, 5, 1, "rbf", 1),                               # a single test row
    _scell(200, 64, 2, "matern52", 64),                       # exact multiples of 64
    _scell(300, 65, 2, "rbf", 129, ls=V.LS2),                 # M one past 64, T one past two column tiles
    _scell(300, 129, 3, "rbf", 70, ls=LS3),                   # M one past 128 (padded to 256)
    _scell(130, 130, 3, "rbf", 65, ls=LS3),                   # M = N
    _scell(400, 257, 3, "matern32", 65),                      # padded to 384
    _scell(8193, 5, 1, "matern32", 130),                      # a second training chunk of the mixture route and of the whitened statistics
    _scell(200, 64, 2, "rbf", 65, tag="ill", ls=[3.0, 3.0], s2=1e-3), _scell(300, 128, 1, "rbf", 65, tag="ill", ls=[2.0], s2=1e-3),
    _scell(130, 17, 1, "composite", 65, tag="co2", block="co2"), _scell(200, 65, 1, "composite", 65, tag="co2", block="co2"),
])
# a second chunk of TEST rows, without covariance: past 8192 in mixture_predict_impl, past 16384 in sgp_predict.  The last chunk is one
# row, and that row is the far point 100 * 1
BIG_T_CELL, BIG_T = "50-5-1-rbf", (8193, 16385)
DRAWS = 9
STREAM_ILL = tuple(n for n in STREAM_CELLS if n.endswith("-ill"))
STREAM_COMPOSITE = tuple(n for n in STREAM_CELLS if "composite" in n)
STREAM_STATIONARY = tuple(n for n in STREAM_CELLS if n not in STREAM_COMPOSITE)
ROUTES = ("whitened", "streaming")


def stream_cells(route):
    """The cells a route is run at: the streaming form everywhere but at the ``ill`` cells."""
    return [n for n in STREAM_CELLS if route == "whitened" or n not in STREAM_ILL]


def stream_cap(name, route):
    return CAP_STREAMING if route == "streaming" else (CAP_TAGGED if name in STREAM_ILL else CAP_UNTAGGED)


# theta_k grows with k, and cond(K_uu) with it: a draw's tolerance is the rule's at its own theta_k, and past draw 0 it may reach
# CAP_TAGGED at any cell.  At the ``ill`` cells the last draws (lengthscales of 3.9 .. 4.2 and 2.8 at s2 = 1.4e-3) lie beyond even that
# in float64 itself: they are judged by the rule alone, and tests/test_stream_predict.py pins which draws these are.
LOOSE_DRAWS = {"200-64-2-rbf-ill": (7, 8), "300-128-1-rbf-ill": (8,)}


def draw_cap(name, k):
    """What the tolerance of draw k may reach on the whitened routes (None: no cap, a LOOSE_DRAWS candidate)."""
    return stream_cap(name, "whitened") if k == 0 else (None if name in STREAM_ILL else CAP_TAGGED)


@functools.lru_cache(maxsize=None)
def stream_inputs(name):
    """The cell's inputs (float64, read-only) by the recipe of ``vfe_reference.cell_inputs``: X, y, Z, kernel, jitter, s2 and ``hyp`` =
    (ls, sf2) or, for a composite kernel, (block, 1.0) -- what CollapsedBound.predict takes as (ls, sf2); ``znoise``: DRAWS x M x d."""
    c = STREAM_CELLS[name]
    N, M, d = c["N"], c["M"], c["d"]
    rs = np.random.RandomState(c["seed"])
    X = rs.standard_normal((N, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rs.standard_normal(N)
    Z = X[rs.permutation(N)[:M]].copy()
    znoise = np.random.RandomState(c["seed"] + 2).standard_normal((DRAWS, M, d))
    hyp = (np.asarray(V._co2(), np.float64), 1.0) if c["kernel"] == "composite" else (np.array(c["ls"], np.float64), c["sf2"])
    for a in (X, y, Z, znoise, hyp[0]):
        a.setflags(write=False)
    return {"X": X, "y": y, "Z": Z, "znoise": znoise, "kernel": c["kernel"], "jitter": c["jitter"], "s2": c["s2"], "hyp": hyp, "T": c["T"]}


@functools.lru_cache(maxsize=None)
def stream_points(name, T=None):
    """The cell's T test points (float64, read-only) by the recipe of ``cell_points``; at a BIG_T size the last row is the far point
    as well.  The leading rows do not depend on T."""
    inp, c = stream_inputs(name), STREAM_CELLS[name]
    T = c["T"] if T is None else T
    Xs = 1.5 * np.random.RandomState(c["seed"] + 1).standard_normal((max(T, 4), c["d"]))
    Xs[0], Xs[1], Xs[2], Xs[3] = inp["X"][0], inp["Z"][0], inp["Z"][-1] + 1e-9, 100.0
    if name == BIG_T_CELL and T in BIG_T:
        Xs[T - 1] = 100.0
    Xs = Xs[:T].copy()
    Xs.setflags(write=False)
    return Xs


def far_rows(name, T=None):
    T = STREAM_CELLS[name]["T"] if T is None else T
    return [r for r in (3,) if r < T] + ([T - 1] if name == BIG_T_CELL and T in BIG_T else [])


def far_is_zero(name, k=0, zs=False):
    """True where k_u* at the far point 100 * 1 underflows to exactly zero in float64 at draw k: the RBF with exp(-r^2 / 2) below the
    denormals for every inducing input (not so at the ``ill`` cells' long lengthscales in one dimension: 1e-307 is left)."""
    Z, hyp, _, _ = draw(name, k, zs)
    return STREAM_CELLS[name]["kernel"] == "rbf" and float(np.exp(-(((100.0 - Z) / hyp) ** 2).sum(1).min() / 2)) == 0.0


def draw(name, k=0, zs=False):
    """(Z_k, ls_k or the block, sf2_k, s2_k) of draw k: theta_k = theta (1 + 0.05 k), ``zs``: Z_k = Z + 0.01 k noise_k."""
    inp = stream_inputs(name)
    f = 1.0 + 0.05 * k
    assert inp["kernel"] != "composite" or k == 0
    Z = inp["Z"] + 0.01 * k * inp["znoise"][k] if zs else inp["Z"]
    return Z, (inp["hyp"][0] * f if k else inp["hyp"][0]), inp["hyp"][1] * f, inp["s2"] * f


def with_cov(T):
    return T <= 1024


def stream_evaluate(name, k=0, zs=False, pred_noise=True, T=None, dtype=LD, order="inverse", mutate=None):
    """``predictive`` / ``predictive_composite`` at draw k of the cell, with the covariance where ``with_cov(T)``."""
    inp, Xs = stream_inputs(name), stream_points(name, T)
    Z, hyp, sf2, s2 = draw(name, k, zs)
    full = with_cov(Xs.shape[0])
    if inp["kernel"] == "composite":
        return predictive_composite(inp["X"], inp["y"], Z, Xs, hyp, s2, inp["jitter"], pred_noise, dtype, order, mutate, full)
    return predictive(inp["X"], inp["y"], Z, Xs, hyp, sf2, s2, inp["jitter"], inp["kernel"], pred_noise, dtype, order, mutate, full)


def stream_keys(name, T=None):
    return COV_KEYS if with_cov(STREAM_CELLS[name]["T"] if T is None else T) else KEYS


@functools.lru_cache(maxsize=None)
def stream_reference(name, k=0, zs=False, pred_noise=True, T=None):
    """(ref, S) of draw k of the cell in long double; computed once per process and never changed."""
    ref, S = stream_evaluate(name, k, zs, pred_noise, T)
    for dct in (ref, S):
        for v in dct.values():
            v.setflags(write=False)
    return ref, S


def streaming64(name, order, pred_noise=True, T=None):
    """The float64 predictive through the UNWHITENED statistics Phi = K_uf K_fu, b = K_uf y at the cell's own theta.  ``order``:
    "oracle" -- oracle.vfe_oracle.predict as it is (for a composite kernel: the same operations on ``comp_k``'s matrices);
    "sandwich" -- W = L^-1 Phi L^-T and q = L_B^-1 L^-1 b from the explicit L^-1, then the explicit L_B^-1: sgp_bound_from_stats's
    ``factors`` as sgp_predict applies them."""
    from scipy.linalg import solve_triangular
    inp, Xs = stream_inputs(name), stream_points(name, T)
    Z, hyp, sf2, s2 = draw(name)
    full, F, M = with_cov(Xs.shape[0]), np.float64, Z.shape[0]
    if order == "oracle" and inp["kernel"] != "composite":
        import torch
        from oracle import vfe_oracle as O
        args = (Xs, inp["X"], inp["y"], Z, hyp, sf2, s2, inp["jitter"], V.KID[inp["kernel"]])
        mu, var = O.predict(*(torch.as_tensor(np.array(a)) if isinstance(a, np.ndarray) else a for a in args), pred_noise=pred_noise)
        got = {"mean": mu.numpy(), "var": var.numpy()}
        if full:
            got["cov"] = O.predict(*(torch.as_tensor(np.array(a)) if isinstance(a, np.ndarray) else a for a in args), full_cov=True,
                                   pred_noise=pred_noise)[1].numpy()
        return got
    if inp["kernel"] == "composite":
        k = lambda rows, cols: CR.comp_k(rows, cols, hyp, F)  # noqa: E731
        sf2 = sum(hyp[a] for a in CR.amp_slots(hyp))
    else:
        k = lambda rows, cols: V._stationary_k(rows, cols, hyp, F(sf2), inp["kernel"], F)  # noqa: E731
    K, Kuf, Kus, I = k(Z, Z) + inp["jitter"] * np.eye(M), k(Z, inp["X"]), k(Z, Xs), np.eye(M)
    Phi, b = Kuf @ Kuf.T, Kuf @ inp["y"]
    if order == "oracle":
        L = np.linalg.cholesky(K)
        W = solve_triangular(L, solve_triangular(L, Phi, lower=True).T, lower=True).T
        u = solve_triangular(L, b, lower=True)
        LB = np.linalg.cholesky(I + 0.5 * (W + W.T) / s2)
        q = solve_triangular(LB, u, lower=True)
        As = solve_triangular(L, Kus, lower=True)
        C = solve_triangular(LB, As, lower=True)
    else:
        Li = tri_inv_ld(chol_ld(K, F), F)
        W = Li @ Phi @ Li.T
        LBi = tri_inv_ld(chol_ld(I + 0.5 * (W + W.T) / s2, F), F)
        q = LBi @ (Li @ b)
        As = Li @ Kus
        C = LBi @ As
    noise = s2 if pred_noise else 0.0
    got = {"mean": C.T @ q / s2, "var": sf2 - (As * As).sum(0) + (C * C).sum(0) + noise}
    if full:
        got["cov"] = k(Xs, Xs) - As.T @ As + C.T @ C + noise * np.eye(Xs.shape[0])
    return got


@functools.lru_cache(maxsize=None)
def stream_e64(name, route="whitened", k=0, zs=False, pred_noise=True, T=None):
    """{key: worst |float64 - long double| / scale} of a route at draw k of the cell: the worse of its two float64 orders.  Measured from
    these float64 runs of the reference alone -- never from a device, never from the fake engine."""
    ref, S = stream_reference(name, k, zs, pred_noise, T)
    keys = stream_keys(name, T)
    if route == "streaming":
        assert k == 0 and not zs and name not in STREAM_ILL
        runs = [streaming64(name, order, pred_noise, T) for order in ("oracle", "sandwich")]
    else:
        runs = [stream_evaluate(name, k, zs, pred_noise, T, np.float64, order)[0] for order in ("inverse", "substitution")]
    e = {key: 0.0 for key in keys}
    for got in runs:
        w = worst(got, ref, S, keys)
        e = {key: max(e[key], w[key]) for key in keys}
    return e


def measure_e64_streaming(name, pred_noise=True, T=None):
    return stream_e64(name, "streaming", 0, False, pred_noise, T)


def stream_tolerances(name, route="whitened", k=0, zs=False, pred_noise=True, T=None):
    return {key: tolerance(v) for key, v in stream_e64(name, route, k, zs, pred_noise, T).items()}
