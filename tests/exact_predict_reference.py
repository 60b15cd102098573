"""Long-double reference of the exact GP predictive (mean and marginal variance per test point) with the condition scale of both, and
of the mixture over draws.

TEST INFRASTRUCTURE ONLY -- numpy ``longdouble`` on the host, the style of tests/exact_batch_reference.py, whose ``chol``,
``tri_inverse`` and ``profile`` it reuses.  It is the yardstick sgp_exact_predict_batch (tests/test_exact_predict_gpu.py) and the CPU
double (tests/exact_predict_double.py) are held against.

    A = sf2 k'(X, X) + s2 I ,  alpha = A^-1 y ,  w_t = A^-1 k*_t ,  mu_t = k*_t^T alpha ,  v_t = sf2 - k*_t^T w_t (+ s2)

First-order condition scales (the same sums with every factor replaced by its absolute value):

    S_mu = |w|^T |A| |alpha| + |k*|^T |alpha| ,   S_v = |w|^T |A| |w| + 2 |k*|^T |w| + sf2

The comparison is |mu - ref| <= TAU S_mu and |v - ref| <= TAU S_v per test point, TAU = 1e-12 of pass2_reference: no factor cond(A).

The mixture's reference evaluates the reduction's formulas in long double FROM THE MOMENTS IT IS GIVEN (the device's own), and returns
the derived rounding bounds of include/sgp_exact_predict.h with eps = 2^-53.
"""
import numpy as np

from exact_batch_reference import LD, TAU, _ld, _ls, chol, profile, tri_inverse  # noqa: F401

EPS = 2.0 ** -53
LOG_2PI = LD("1.8378770664093454835606594728112352797")


def reference(X, y, Xs, ls, sf2, s2, kernel="rbf", pred_noise=True):
    """dict(mean [T], var [T], S_mu [T], S_v [T], cond, info) -- long double, cond in float64."""
    X, y, Xs = _ld(X), _ld(y).reshape(-1), _ld(Xs)
    N, d = X.shape
    ls = _ls(ls, d)
    sf2, s2 = LD(float(sf2)), LD(float(s2))
    diff = (X[:, None, :] - X[None, :, :]) / ls
    A = sf2 * profile((diff * diff).sum(-1), kernel)[0] + s2 * np.eye(N, dtype=LD)
    L, info = chol(A)
    if info:
        return {"info": info}
    Li = tri_inverse(L)
    Ainv = Li.T @ Li
    alpha = Ainv @ y
    ds = (X[:, None, :] - Xs[None, :, :]) / ls
    Ks = sf2 * profile((ds * ds).sum(-1), kernel)[0]          # N x T
    W = Ainv @ Ks                                             # N x T
    mean = Ks.T @ alpha
    var = sf2 - (Ks * W).sum(0) + (s2 if pred_noise else LD(0))
    aA = np.abs(A)
    S_mu = np.abs(W).T @ (aA @ np.abs(alpha)) + np.abs(Ks).T @ np.abs(alpha)
    S_v = (np.abs(W) * (aA @ np.abs(W))).sum(0) + 2 * (np.abs(Ks) * np.abs(W)).sum(0) + sf2
    ev = np.linalg.eigvalsh(A.astype(np.float64))
    return {"mean": mean, "var": var, "S_mu": S_mu, "S_v": S_v, "cond": float(ev[-1] / ev[0]), "info": 0}


def ratios(mean, var, ref):
    """(max |mean - ref| / S_mu, max |var - ref| / S_v) over the test points."""
    rm = np.abs(_ld(mean).reshape(-1) - ref["mean"]) / ref["S_mu"]
    rv = np.abs(_ld(var).reshape(-1) - ref["var"]) / ref["S_v"]
    rm = np.where(np.abs(_ld(mean).reshape(-1) - ref["mean"]) == 0, LD(0), rm)  # (S_mu = 0 where alpha = 0: must be exact)
    return float(np.nan_to_num(rm.astype(np.float64), nan=np.inf).max()), float(np.nan_to_num(rv.astype(np.float64), nan=np.inf).max())


def assert_close(mean, var, ref, tau=TAU, what=""):
    rm, rv = ratios(mean, var, ref)
    assert rm <= tau, "%s: worst |mean - ref| / S_mu = %.3e > %.1e (cond %.3g)" % (what, rm, tau, ref["cond"])
    assert rv <= tau, "%s: worst |var - ref| / S_v = %.3e > %.1e (cond %.3g)" % (what, rv, tau, ref["cond"])
    return rm, rv


def mixture_reference(mean, var, info, y=None):
    """One group: mean / var are n_draws x T (float64, the moments under test), info n_draws, y T or None.  Returns long-double
    dict(mean, var, logpdf, mean_logpdf [T], kept) and ``bounds``: the derived rounding bounds of each, float64 [T]."""
    keep = np.asarray(info).reshape(-1) == 0
    mu, v = _ld(np.asarray(mean)[keep]), _ld(np.asarray(var)[keep])
    n, T = mu.shape[0], np.asarray(mean).shape[1]
    if n == 0:
        nan = np.full(T, np.nan)
        return {"mean": nan, "var": nan, "logpdf": nan, "mean_logpdf": nan, "kept": 0, "bounds": None}
    m = mu.sum(0) / n
    spread = v + (mu - m) ** 2
    out = {"mean": m, "var": spread.sum(0) / n, "kept": n, "logpdf": None, "mean_logpdf": None}
    bounds = {"mean": EPS * (n + 2) * np.abs(mu).max(0).astype(np.float64),
              "var": 2 * EPS * (n + 4) * spread.max(0).astype(np.float64)}
    if y is not None:
        y = _ld(y).reshape(-1)
        q = (y - mu) ** 2 / (2 * v)
        half_log = (LOG_2PI + np.log(v)) / 2
        l = -half_log - q
        mx = l.max(0)
        out["logpdf"] = mx + np.log(np.exp(l - mx).sum(0) / n)
        out["mean_logpdf"] = l.sum(0) / n
        c = (np.abs(half_log) + q).max(0).astype(np.float64)
        bounds["logpdf"] = EPS * (8 * c + n + 8)
        bounds["mean_logpdf"] = EPS * (8 + n) * c
    out["bounds"] = bounds
    return out


def assert_mixture_close(got, ref, what=""):
    """got: dict of float64 arrays [T] (mean, var, and logpdf / mean_logpdf where the reference has them)."""
    worst = {}
    for k, b in ref["bounds"].items():
        err = np.abs(_ld(got[k]) - ref[k]).astype(np.float64)
        assert np.all(np.isfinite(np.asarray(got[k]))), "%s: %s is not finite" % (what, k)
        worst[k] = float((err / b).max())
        assert np.all(err <= b), "%s: %s off by %.3e of its bound" % (what, k, worst[k])
    return worst
