"""Batched exact-GP marginal likelihood on top of ``engine.exact_eval_batch``: LML surfaces and multi-start ML-II.

``lml_surface`` is the reference's nested loops over ``gp.log_marginal_likelihood(log theta)`` (experiments/lml_surface.py,
experiments/hyperparameter_identification.py) as ONE launch; ``fit_ml2`` is scikit-learn's ``GaussianProcessRegressor(
n_restarts_optimizer=R).fit`` for B data sets x (1 + R) starts as ONE batched optimisation.  torch is plumbing: the optimiser's state
lives in tensors on the engine's device, every trial point of every problem is one row of one ``exact_eval_batch``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ._lib import KERNEL_IDS

MAX_N, MAX_D = 128, 8


def _engine(engine):
    if engine is not None:
        return engine
    from .engine import HipEngine
    return HipEngine()


def _dev(a, engine):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(engine.device).contiguous()


def _check_kernel(kernel):
    if kernel not in KERNEL_IDS or kernel == "composite":
        raise ValueError("kernel must be one of rbf, matern32, matern52 (got %r)" % (kernel,))


def _check_data(X, N_of_y):
    if X.ndim != 2 or not 1 <= X.shape[0] <= MAX_N or not 1 <= X.shape[1] <= MAX_D:
        raise ValueError("X must be N x d with 1 <= N <= %d and 1 <= d <= %d (got %s)" % (MAX_N, MAX_D, X.shape))
    if N_of_y != X.shape[0]:
        raise ValueError("y has %d entries for %d rows of X" % (N_of_y, X.shape[0]))


def lml_surface(X, y, sf2, ls, s2, kernel="rbf", engine=None):
    """log N(y | 0, sf2 k(X, X; ls) + s2 I) at every cell of a grid of hyper-parameters, in one launch.

    ``sf2``, ``ls`` and ``s2`` broadcast against each other.  ``ls`` is one lengthscale per cell (shared by the d dimensions) or, for
    d > 1, carries a trailing axis of length d (ARD) that takes no part in the broadcast.  Returns a float64 numpy array of the broadcast
    shape; a cell whose matrix is not numerically positive definite (``info != 0``) is NaN."""
    _check_kernel(kernel)
    X = np.asarray(X, dtype=np.float64)
    X = X[:, None] if X.ndim == 1 else X
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    _check_data(X, y.size)
    d = X.shape[1]
    sf2, ls, s2 = (np.asarray(v, dtype=np.float64) for v in (sf2, ls, s2))
    ard = d > 1 and ls.ndim >= 1 and ls.shape[-1] == d
    try:
        shape = np.broadcast_shapes(sf2.shape, s2.shape, ls.shape[:-1] if ard else ls.shape)
    except ValueError:
        raise ValueError("sf2 %s, ls %s and s2 %s do not broadcast" % (sf2.shape, ls.shape, s2.shape)) from None
    ls_full = np.broadcast_to(ls if ard else ls[..., None], shape + (d,))
    theta = np.concatenate([ls_full, np.broadcast_to(sf2, shape)[..., None], np.broadcast_to(s2, shape)[..., None]], -1).reshape(-1, d + 2)
    if theta.shape[0] == 0:
        return np.zeros(shape)
    eng = _engine(engine)
    F, _, _, _ = eng.exact_eval_batch(_dev(X, eng), _dev(y, eng), _dev(theta, eng), kernel=kernel, want_grad=False)
    return F.cpu().numpy().reshape(shape)  # (the entry point writes NaN where info != 0)


@dataclass
class Ml2Result:
    """``fit_ml2``'s result (numpy).  theta rows are [ls_1..d | sf2 | s2]."""
    theta: np.ndarray       # B x (d + 2): the best start of every data set
    lml: np.ndarray         # B
    n_evals: np.ndarray     # B: evaluations spent on the data set's starts (each one row of a batched evaluation)
    theta_all: np.ndarray   # B x (1 + R) x (d + 2)
    lml_all: np.ndarray     # B x (1 + R)
    converged: np.ndarray   # B x (1 + R) bool
    n_iter: np.ndarray      # B x (1 + R): accepted L-BFGS steps
    n_batches: int          # batched evaluations (launches) of the whole fit
    # what the fit was made with (``fit_ml2`` fills them in): ``predict`` needs them
    X: Optional[np.ndarray] = None   # N x d or B x N x d
    Y: Optional[np.ndarray] = None   # B x N
    kernel: Optional[str] = None
    engine: object = None

    def predict(self, X_test, Y_test=None, pred_noise=True, probs=None):
        """The plug-in predictive at ``theta`` (``exact_predict.ExactMixturePredictive`` with S = 1; theta is constrained already: no
        exp, no noise floor)."""
        if self.X is None or self.Y is None or self.kernel is None:
            raise ValueError("this result does not carry the data it was fitted to (X, Y, kernel)")
        from .exact_predict import predict_theta_batch
        return predict_theta_batch(self.X, self.Y, self.theta[:, None, :], X_test, Y_test, kernel=self.kernel, pred_noise=pred_noise,
                                   engine=self.engine, probs=probs)


MEMORY, MAX_ITER, PGTOL, FTOL, ARMIJO = 10, 200, 1e-5, 2.2e-9, 1e-4  # FTOL: scipy's factr = 1e7 times 2.2e-16
MIN_STEP = 2.0 ** -40
PG_NEAR = 5e-5  # 5 x PGTOL (fit_ml2's stopping rule)


def draw_starts(bounds_log, free, B, R, seed):
    """R restart points per data set, log-uniform inside the bounds -- scikit-learn's rule (``rng.uniform(log lo, log hi)`` over the
    free hyper-parameters in ITS order [sf2 | ls_1..d | s2], one draw per restart), data set after data set from one RandomState(seed).
    Returns log theta, B x R x (d + 2) in this module's order, NaN in the components that are not free."""
    n = bounds_log.shape[0]
    order = [n - 2] + list(range(n - 2)) + [n - 1]
    order = [i for i in order if free[i]]
    rng = np.random.RandomState(seed)
    out = np.full((B, R, n), np.nan)
    for b in range(B):
        for r in range(R):
            out[b, r, order] = rng.uniform(bounds_log[order, 0], bounds_log[order, 1])
    return out


def fit_ml2(X, Y, kernel="rbf", noise="learn", theta0=None, bounds=None, n_restarts=10, starts=None, seed=None, engine=None,
            max_iter=MAX_ITER):
    """Type-II maximum likelihood for B data sets from 1 + R starts each, as one batched projected L-BFGS over log theta.

    X: N x d (shared) or B x N x d;  Y: B x N (or N).  ``theta0`` ([ls_1..d | sf2 | s2], or B rows of it) is every data set's first
    start; ``bounds`` is (d + 2) x 2 (lower, upper) in the same units.  ``noise="fixed"`` keeps s2 at theta0's value (the optimiser masks
    that component; the kernel does not know).  ``starts`` (R x (d + 2) or B x R x (d + 2)) gives the restarts, default: ``n_restarts``
    log-uniform draws inside the bounds from ``RandomState(seed)`` (``draw_starts``).

    The optimiser: memory 10, projection onto the box, Armijo backtracking (c1 = 1e-4, halving).  A problem has converged when the
    infinity-norm of its projected gradient is <= 1e-5, or when a full quasi-Newton step (not a shortened one, not a steepest-descent
    stride: their small gain says nothing about the distance to the optimum) decreases -LML by <= 2.2e-9 relative while the projected
    gradient is <= 5e-5 -- further out such a step is a flat direction the curvature pairs have not described yet, and the problem goes
    on.  It stops unconverged after ``max_iter`` accepted steps; a stopped problem is frozen.  Problems advance independently -- in a
    round some evaluate a first trial of a new direction, others a shortened step -- so a round is ONE ``exact_eval_batch`` and one
    host synchronisation (is anything still active?).
    """
    _check_kernel(kernel)
    if noise not in ("learn", "fixed"):
        raise ValueError("noise must be 'learn' or 'fixed' (got %r)" % (noise,))
    if theta0 is None or bounds is None:
        raise ValueError("theta0 and bounds are required")
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y[None] if Y.ndim == 1 else Y
    if Y.ndim != 2:
        raise ValueError("Y must be B x N")
    B, N = Y.shape
    X = X[:, None] if X.ndim == 1 else X
    Xs = X if X.ndim == 3 else X[None]
    if Xs.ndim != 3 or Xs.shape[0] not in (1, B):
        raise ValueError("X must be N x d or B x N x d (got %s for B = %d)" % (X.shape, B))
    _check_data(Xs[0], N)
    d = Xs.shape[2]
    n = d + 2
    theta0 = np.asarray(theta0, dtype=np.float64)
    bounds = np.asarray(bounds, dtype=np.float64)
    if theta0.shape not in ((n,), (B, n)) or bounds.shape != (n, 2):
        raise ValueError("theta0 must have %d entries (or B rows of them) and bounds must be %d x 2" % (n, n))
    if not (np.all(bounds > 0) and np.all(bounds[:, 0] <= bounds[:, 1]) and np.all(theta0 > 0)):
        raise ValueError("theta0 and bounds must be positive, lower <= upper")
    free = np.ones(n, dtype=bool)
    if noise == "fixed":
        free[n - 1] = False
    z0 = np.broadcast_to(np.log(theta0), (B, n))
    blog = np.log(bounds)
    if starts is None:
        R = int(n_restarts)
        if R < 0:
            raise ValueError("n_restarts must be >= 0")
        zs = draw_starts(blog, free, B, R, seed)
    else:
        st = np.asarray(starts, dtype=np.float64)
        st = np.broadcast_to(st, (B,) + st.shape) if st.ndim == 2 else st
        if st.ndim != 3 or st.shape[0] != B or st.shape[2] != n:
            raise ValueError("starts must be R x %d or B x R x %d" % (n, n))
        R = st.shape[1]
        with np.errstate(invalid="ignore", divide="ignore"):
            zs = np.log(st)
    zall = np.concatenate([z0[:, None, :], zs], 1)                      # B x (1 + R) x n
    zall = np.where(free, zall, z0[:, None, :])                         # a fixed component keeps theta0's value in every start
    if not np.all(np.isfinite(zall)):
        raise ValueError("starts must be positive and finite")
    S1 = 1 + R
    Q = B * S1
    eng = _engine(engine)
    dev = eng.device
    Xd, Yd = _dev(Xs, eng), _dev(Y, eng)
    set_of = torch.arange(B, dtype=torch.int32).repeat_interleave(S1).to(dev).contiguous()
    ix = set_of if Xs.shape[0] == B and B > 1 else None
    freem = torch.as_tensor(free).to(dev)
    lo = torch.where(freem, _dev(blog[:, 0], eng), torch.full((n,), -np.inf, dtype=torch.float64, device=dev))
    hi = torch.where(freem, _dev(blog[:, 1], eng), torch.full((n,), np.inf, dtype=torch.float64, device=dev))
    z = _dev(zall.reshape(Q, n), eng)
    z = torch.where(freem, torch.minimum(torch.maximum(z, lo), hi), z)

    def evaluate(zq):
        th = torch.exp(zq).contiguous()
        F, _, g, info = eng.exact_eval_batch(Xd, Yd, th, ix=ix, iy=set_of, kernel=kernel, want_grad=True)
        f = -F
        gz = torch.where(freem, -th * g, torch.zeros_like(g))           # d(-F)/d log theta; a fixed component does not move
        ok = (info == 0) & torch.isfinite(f) & torch.isfinite(gz).all(1)
        return torch.where(ok, f, torch.full_like(f, np.inf)), torch.where(ok[:, None], gz, torch.zeros_like(gz)), ok

    def proj_grad(zq, gq):
        return zq - torch.minimum(torch.maximum(zq - gq, lo), hi)

    def direction(g, z, Sh, Yh, rho):
        """-H g of the two-loop recursion over the free, inactive components; steepest descent where that is no descent direction."""
        act = ((z <= lo) & (g > 0)) | ((z >= hi) & (g < 0)) | ~freem
        gm = torch.where(act, torch.zeros_like(g), g)
        q = gm.clone()
        al = []
        for i in range(MEMORY - 1, -1, -1):
            a = rho[:, i] * (Sh[:, i] * q).sum(1)
            q = q - a[:, None] * Yh[:, i]
            al.append(a)
        al.reverse()
        yy = (Yh[:, -1] * Yh[:, -1]).sum(1)
        gamma = torch.where(rho[:, -1] > 0, 1.0 / (rho[:, -1] * yy).clamp_min(1e-300), torch.ones_like(yy))
        r = gamma[:, None] * q
        for i in range(MEMORY):
            b = rho[:, i] * (Yh[:, i] * r).sum(1)
            r = r + Sh[:, i] * (al[i] - b)[:, None]
        dirn = torch.where(act, torch.zeros_like(r), -r)
        slope = (dirn * g).sum(1)
        gn = gm.norm(dim=1)
        steep = ~(slope < -1e-16 * gn * dirn.norm(dim=1)) | ~torch.isfinite(slope)
        first = (rho[:, -1] == 0) | steep
        dirn = torch.where(steep[:, None], -gm, dirn)
        # the first step of a history has unit length in log theta (scipy's L-BFGS-B starts the same way).  Where -LML is concave -- the
        # plateau at a tiny amplitude -- no curvature pair is accepted and every step is such a step: the plateau is crossed in strides.
        t0 = torch.where(first, 1.0 / gn.clamp_min(1e-300), torch.ones_like(gn))
        return dirn, t0, steep, ~first

    f, g, ok = evaluate(z)
    n_evals = torch.ones(Q, dtype=torch.int64, device=dev)
    n_iter = torch.zeros(Q, dtype=torch.int64, device=dev)
    Sh = torch.zeros(Q, MEMORY, n, dtype=torch.float64, device=dev)
    Yh = torch.zeros_like(Sh)
    rho = torch.zeros(Q, MEMORY, dtype=torch.float64, device=dev)
    converged = ok & (proj_grad(z, g).abs().amax(1) <= PGTOL)
    active = ok & ~converged                                               # a start that cannot be evaluated is reported, not optimised
    dirn, t, _, qn = direction(g, z, Sh, Yh, rho)
    n_batches = 1
    while n_batches < 4 * max_iter + 50:
        if not bool(active.any()):                                         # the round's one host synchronisation
            break
        z_try = torch.where(active[:, None], torch.minimum(torch.maximum(z + t[:, None] * dirn, lo), hi), z)
        f_try, g_try, ok = evaluate(z_try)
        n_batches += 1
        n_evals += active.to(torch.int64)
        step = z_try - z
        accept = active & ok & (f_try <= f + ARMIJO * (g * step).sum(1))
        reject = active & ~accept
        # accepted: curvature pair, state, convergence
        yv = g_try - g
        sy = (step * yv).sum(1)
        keep = accept & (sy > 1e-10 * (yv * yv).sum(1)) & (sy > 0)
        kk = keep[:, None, None]
        Sh = torch.where(kk, torch.cat([Sh[:, 1:], step[:, None, :]], 1), Sh)
        Yh = torch.where(kk, torch.cat([Yh[:, 1:], yv[:, None, :]], 1), Yh)
        rho = torch.where(keep[:, None], torch.cat([rho[:, 1:], (1.0 / sy.clamp_min(1e-300))[:, None]], 1), rho)
        decr = f - f_try
        small = qn & (t == 1.0) & (decr <= FTOL * torch.maximum(torch.maximum(f.abs(), f_try.abs()), torch.ones_like(f)))
        z = torch.where(accept[:, None], z_try, z)
        g = torch.where(accept[:, None], g_try, g)
        f = torch.where(accept, f_try, f)
        n_iter += accept.to(torch.int64)
        pgn = proj_grad(z, g).abs().amax(1)
        done_ok = accept & ((pgn <= PGTOL) | (small & (pgn <= PG_NEAR)))
        converged = converged | done_ok
        new_dirn, t0, steep, new_qn = direction(g, z, Sh, Yh, rho)
        wipe = (accept & steep)[:, None]
        rho = torch.where(wipe, torch.zeros_like(rho), rho)
        dirn = torch.where(accept[:, None], new_dirn, dirn)
        t = torch.where(accept, t0, t)
        qn = torch.where(accept, new_qn, qn)
        # rejected: halve; a step that has shrunk to nothing restarts once from steepest descent, then gives up
        t = torch.where(reject, 0.5 * t, t)
        dead = reject & (t * dirn.abs().amax(1) < MIN_STEP)
        had_hist = rho[:, -1] > 0
        restart = dead & had_hist
        rho = torch.where(restart[:, None], torch.zeros_like(rho), rho)
        sd, sd_t, _, _ = direction(g, z, Sh, Yh, rho)
        dirn = torch.where(restart[:, None], sd, dirn)
        t = torch.where(restart, sd_t, t)
        qn = qn & ~restart
        gave_up = dead & ~had_hist
        active = active & ~done_ok & ~gave_up & (n_iter < max_iter)
    theta_all = torch.exp(z).reshape(B, S1, n).cpu().numpy()
    lml_all = (-f).reshape(B, S1).cpu().numpy()
    lml_all = np.where(np.isfinite(lml_all), lml_all, np.nan)             # a start that could not be evaluated
    conv = converged.reshape(B, S1).cpu().numpy()
    score = np.where(np.isfinite(lml_all), lml_all, -np.inf)
    best = score.argmax(1)
    rows = np.arange(B)
    return Ml2Result(theta=theta_all[rows, best], lml=lml_all[rows, best], n_evals=n_evals.reshape(B, S1).sum(1).cpu().numpy(),
                     theta_all=theta_all, lml_all=lml_all, converged=conv, n_iter=n_iter.reshape(B, S1).cpu().numpy(),
                     n_batches=n_batches, X=Xs if Xs.shape[0] == B and B > 1 else Xs[0], Y=Y, kernel=kernel, engine=eng)


def identification_data(n_train, n_sets, rng, sig_sd=5.0, lengthscale=2.0, noise_sd=1.0, uniform=True, d=1, n_grid=500, latent=None):
    """The data of the hyper-parameter identification study: ``n_sets`` draws of a zero-mean GP prior (amplitude ``sig_sd``, RBF
    lengthscale ``lengthscale``) on a grid of ``n_grid`` points of [0, 10]^d, observed with N(0, noise_sd^2) noise at ``n_train`` grid
    points shared by all the sets -- chosen uniformly, or (``uniform=False``, d = 1) from an equal mixture of N(2, 1) and N(8, 1), in
    both cases without replacement.  d = 1: the regular grid; d > 1: uniform random grid points.  ``latent=(X_all, f_all)`` reuses a
    prior draw (the study observes the same functions at every size and noise level).  Returns (X [n_train x d], Y [n_sets x n_train],
    (X_all, f_all)).  ``rng`` is a numpy Generator."""
    if latent is None:
        X_all = np.linspace(0.0, 10.0, n_grid)[:, None] if d == 1 else rng.uniform(0.0, 10.0, (n_grid, d))
        diff = (X_all[:, None, :] - X_all[None, :, :]) / lengthscale
        K = sig_sd ** 2 * np.exp(-0.5 * (diff * diff).sum(-1))
        w, V = np.linalg.eigh(K)                                          # (K is numerically singular: no Cholesky)
        f_all = (V * np.sqrt(np.maximum(w, 0.0))) @ rng.standard_normal((n_grid, n_sets))
        f_all = f_all.T
    else:
        X_all, f_all = latent
    n_grid = X_all.shape[0]
    if uniform or d > 1:
        idx = rng.choice(n_grid, n_train, replace=False)
    else:
        x = X_all[:, 0]
        pdf = 0.5 * np.exp(-0.5 * (x - 2.0) ** 2) + 0.5 * np.exp(-0.5 * (x - 8.0) ** 2)
        idx = rng.choice(n_grid, n_train, replace=False, p=pdf / pdf.sum())
    Y = f_all[:n_sets, idx] + noise_sd * rng.standard_normal((n_sets, n_train))
    return X_all[idx].copy(), Y, (X_all, f_all)
