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

``mutate`` breaks one thing at a time (MUTATIONS) so that a test can show the comparison failing on it.

The cells are those of ``vfe_batch_double.CELLS`` with N <= 3000; a cell's test points are T = TN + 3 rows (TN the tile of the cell's
size class: two tiles, the last of three points): 1.5 x standard normal, row 0 the training row X[0], row 1 the inducing input Z[0], row 2
Z[-1] + 1e-9, row 3 the point 100 * 1 (mean exactly 0, var = sf2 (+ s2)).
"""
import functools

import numpy as np

import vfe_batch_double as VB
import vfe_reference as V
from vfe_reference import LD, UNDERFLOW, chol_ld, tolerance, tri_inv_ld  # noqa: F401

MUTATIONS = ("no_v2", "no_jitter", "no_noise")
CELLS = [n for n in VB.CELLS if VB.spec(n)["N"] <= 3000]
TAGGED = ("200-64-2-rbf-ill", "200-33-2-matern32-near", "200-64-2-rbf-sf100")
KEYS = ("mean", "var")
CAP_UNTAGGED, CAP_TAGGED = 1e-10, 1e-8  # what tol may reach at a cell (tests/test_vfe_predict.py): the rule cannot hide a failure


def tile_rows(M):
    """vb_tile_rows of M's size class (csrc/sgp_vfe_batch.hpp): 128 / 64 / 32 test points per tile."""
    return 2048 // (16 if M <= 16 else 32 if M <= 32 else 64)


def predictive(X, y, Z, Xs, ls, sf2, s2, jitter, kernel, pred_noise=True, dtype=LD, order="inverse", mutate=None):
    """(ref, S): dicts with mean [T], var [T] in ``dtype`` -- S the condition scale of each."""
    assert mutate is None or mutate in MUTATIONS
    F = dtype
    X, y, Z, Xs = V._c(X, F), V._c(y, F).reshape(-1), V._c(Z, F), V._c(Xs, F)
    d, M = X.shape[1], Z.shape[0]
    ls = V._c(ls, F).reshape(-1)
    ls = np.repeat(ls, d) if ls.size == 1 and d > 1 else ls
    sf2, s2, J = F(V._c(sf2, F)), F(V._c(s2, F)), F(V._c(jitter, F))
    K = V._stationary_k(Z, Z, ls, sf2, kernel, F) + (0 if mutate == "no_jitter" else J) * np.eye(M, dtype=F)
    Kuf = V._stationary_k(Z, X, ls, sf2, kernel, F)
    Kus = V._stationary_k(Z, Xs, ls, sf2, kernel, F)
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
    v = fwdB(a)
    noise = s2 if pred_noise and mutate != "no_noise" else F(0)
    a2, v2 = (a * a).sum(0), (F(0) * a[0] if mutate == "no_v2" else (v * v).sum(0))
    ref = {"mean": (a * g[:, None]).sum(0) / s2, "var": sf2 - a2 + v2 + noise}
    S = {"mean": (np.abs(a) * np.abs(g)[:, None]).sum(0) / s2, "var": sf2 + a2 + (v * v).sum(0) + (s2 if pred_noise else F(0))}
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


def worst(got, ref, S):
    """{mean, var: worst |got - ref| / S over the test points}, UNDERFLOW the only allowance (``vfe_reference.worst``)."""
    return V.worst(got, ref, S, KEYS)


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
