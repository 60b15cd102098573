"""Long-double reference of the exact GP marginal likelihood and its gradient, with the condition scale of every output.

TEST INFRASTRUCTURE ONLY -- numpy ``longdouble`` (x87 extended: eps 1.1e-19) on the host, the style of tests/pass2_reference.py.  It is the
yardstick sgp_exact_eval_batch (tests/test_exact_batch_gpu.py) and the CPU double (tests/exact_batch_double.py) are held against.

    A = sf2 k'(X, X) + s2 I ,  alpha = A^-1 y ,  F = -1/2 y^T alpha - 1/2 log|A| - N/2 log 2 pi
    g[theta] = 1/2 sum (alpha alpha^T - A^-1) o dA/dtheta ,   theta = [ls_1..d | sf2 | s2]   (the lengthscale itself, not its log)

Condition scales (the same sums with every factor replaced by its absolute value):

    S_F        = 1/2 (|alpha|^T |A| |alpha| + sum |A^-1| o |A|)
    S_g[theta] = 1/2 sum (|alpha| |alpha|^T + |A^-1|) o |dA/dtheta|

A relative perturbation delta of A's entries moves F by at most delta S_F to first order, and the gradient by delta kappa_2(A) S_g (it
goes through A^-1 twice).  The comparison everywhere is  |F - ref| <= TAU S_F  and  |g - ref| <= TAU kappa_2(A) S_g  component-wise,
TAU = 1e-12 of pass2_reference.
"""
import numpy as np

from pass2_reference import LD, TAU, _ld, _ls, profile  # noqa: F401

UNDERFLOW = LD(1e-290)
LOG_2PI = LD("1.8378770664093454835606594728112352797")


def chol(A):
    """Lower Cholesky factor in long double, or None with the 1-based index of the first non-positive pivot."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            return None, j + 1
        L[j:, j] = v / np.sqrt(v[0])
    return L, 0


def tri_inverse(L):
    n = L.shape[0]
    Li = np.zeros_like(L)
    for i in range(n):
        Li[i, i] = 1 / L[i, i]
        if i:
            Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
    return Li


def reference(X, y, ls, sf2, s2, kernel="rbf"):
    """dict(F, quad, logdet, trinv, g [d + 2], S_F, S_g [d + 2], cond, info) -- long double, cond in float64."""
    X, y = _ld(X), _ld(y).reshape(-1)
    N, d = X.shape
    ls = _ls(ls, d)
    sf2, s2 = LD(float(sf2)), LD(float(s2))
    diff = (X[:, None, :] - X[None, :, :]) / ls
    D = diff * diff
    kp, hp = profile(D.sum(-1), kernel)
    A = sf2 * kp + s2 * np.eye(N, dtype=LD)
    L, info = chol(A)
    if info:
        return {"info": info, "F": np.nan}
    Li = tri_inverse(L)
    Ainv = Li.T @ Li
    alpha = Ainv @ y
    quad = y @ alpha
    logdet = 2 * np.log(np.diagonal(L)).sum()
    F = -quad / 2 - logdet / 2 - N * LOG_2PI / 2
    G = np.outer(alpha, alpha) - Ainv
    Gabs = np.outer(np.abs(alpha), np.abs(alpha)) + np.abs(Ainv)
    dA = [sf2 * hp * (-2 * D[:, :, q] / ls[q]) for q in range(d)] + [kp, np.eye(N, dtype=LD)]
    g = np.array([(G * dq).sum() / 2 for dq in dA], dtype=LD)
    S_g = np.array([(Gabs * np.abs(dq)).sum() / 2 for dq in dA], dtype=LD)
    S_F = (np.abs(alpha) @ np.abs(A) @ np.abs(alpha) + (np.abs(Ainv) * np.abs(A)).sum()) / 2
    ev = np.linalg.eigvalsh(A.astype(np.float64))
    return {"F": F, "quad": quad, "logdet": logdet, "trinv": np.trace(Ainv), "g": g, "S_F": S_F, "S_g": S_g,
            "cond": float(ev[-1] / ev[0]), "info": 0}


def ratios(F, g, ref):
    """(|F - ref| / S_F, max |g - ref| / (kappa_2 S_g)); g may be None."""
    rF = float(abs(LD(float(F)) - ref["F"]) / ref["S_F"])
    if g is None:
        return rF, 0.0
    # long double keeps terms (exp(-5000) at a short lengthscale) that lie below the whole float64 range: that much is no error
    err = np.maximum(np.abs(_ld(g).reshape(-1) - ref["g"]) - UNDERFLOW, 0)
    with np.errstate(divide="ignore", invalid="ignore"):  # a component without a single term (S_g = 0, e.g. N = 1) must be exact
        r = np.where(err == 0, LD(0), err / (LD(ref["cond"]) * ref["S_g"]))
    r = np.where(np.isnan(r), LD(np.inf), r)
    return rF, float(r.max())


def assert_close(F, g, ref, tau=TAU, what=""):
    rF, rg = ratios(F, g, ref)
    assert np.isfinite(rF) and rF <= tau, "%s: |F - ref| / S_F = %.3e > %.1e (F %.17g, ref %.17g, cond %.3g)" % (
        what, rF, tau, float(F), float(ref["F"]), ref["cond"])
    assert np.isfinite(rg) and rg <= tau, "%s: worst |g - ref| / (cond S_g) = %.3e > %.1e (cond %.3g)" % (what, rg, tau, ref["cond"])
    return rF, rg
