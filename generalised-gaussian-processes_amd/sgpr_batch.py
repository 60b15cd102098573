"""Batched collapsed (VFE) sparse-GP bound on top of ``engine.vfe_eval_batch``: ELBO surfaces and lock-step training of many
``SparseGPR`` problems.

``elbo_surface`` is the sparse counterpart of ``ml2.lml_surface``: the bound at every cell of a grid of hyper-parameters in ONE launch.
``fit_sgpr_batch`` is ``SparseGPR.train_model`` (softplus parameters, loss -F / N, torch's Adam) for B data sets x (1 + R) starts as ONE
batched optimisation with one launch per step.  torch is plumbing: parameters and optimiser state are tensors on the engine's device,
every problem is one row of one ``vfe_eval_batch``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from ._lib import VFE_BATCH_MAX_D as MAX_D, VFE_BATCH_MAX_M as MAX_M, VFE_BATCH_MAX_N as MAX_N
from .gp_shim import NOISE_FLOOR
from .ml2 import _check_kernel, _dev, _engine

ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8   # torch.optim.Adam's defaults, which the reference's training loop uses


def _check_sparse_data(X, N_of_y, Z):
    if X.ndim != 2 or not 1 <= X.shape[0] <= MAX_N or not 1 <= X.shape[1] <= MAX_D:
        raise ValueError("X must be N x d with 1 <= N <= %d and 1 <= d <= %d (got %s)" % (MAX_N, MAX_D, X.shape))
    if N_of_y != X.shape[0]:
        raise ValueError("y has %d entries for %d rows of X" % (N_of_y, X.shape[0]))
    if Z.ndim != 2 or not 1 <= Z.shape[0] <= MAX_M or Z.shape[1] != X.shape[1]:
        raise ValueError("Z must be M x %d with 1 <= M <= %d (got %s)" % (X.shape[1], MAX_M, Z.shape))


def elbo_surface(X, y, Z, sf2, ls, s2, kernel="rbf", jitter=1e-6, parts=False, engine=None):
    """The collapsed bound F(sf2, ls, s2) of the sparse GP with inducing inputs Z at every cell of a grid of hyper-parameters, in one
    launch.

    ``sf2``, ``ls`` and ``s2`` broadcast against each other by ``lml_surface``'s rules: ``ls`` is one lengthscale per cell (shared by
    the d dimensions) or, for d > 1, carries a trailing axis of length d (ARD) that takes no part in the broadcast.  Returns a float64
    numpy array of the broadcast shape -- with ``parts`` the tuple (F, logmarg, trace), F = logmarg - trace; a cell that the kernel
    reports as not numerically positive definite (``info != 0``) is NaN."""
    _check_kernel(kernel)
    X = np.asarray(X, dtype=np.float64)
    X = X[:, None] if X.ndim == 1 else X
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    Z = np.asarray(Z, dtype=np.float64)
    Z = Z[:, None] if Z.ndim == 1 else Z
    _check_sparse_data(X, y.size, Z)
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
        return (np.zeros(shape),) * 3 if parts else np.zeros(shape)
    eng = _engine(engine)
    out, _, _ = eng.vfe_eval_batch(_dev(X, eng), _dev(y, eng), _dev(Z, eng), _dev(theta, eng), kernel=kernel, jitter=jitter, want_grad=False)
    out = out.cpu().numpy()  # (the entry point writes NaN where info != 0)
    if parts:
        return tuple(out[:, c].reshape(shape) for c in (0, d + 3, d + 4))
    return out[:, 0].reshape(shape)


@dataclass
class SgprBatchResult:
    """What ``fit_sgpr_batch`` returns (numpy).  theta rows are [ls_1..d | sf2 | s2] (s2 includes the 1e-4 floor of the likelihood)."""
    theta: np.ndarray        # B x (d + 2): the best start of every data set by final F
    Z: np.ndarray            # B x M x d
    elbo: np.ndarray         # B
    best: np.ndarray         # B: the index of that start
    theta_all: np.ndarray    # B x (1 + R) x (d + 2)
    Z_all: np.ndarray        # B x (1 + R) x M x d
    elbo_all: np.ndarray     # B x (1 + R): NaN where the final evaluation failed
    losses: np.ndarray       # steps x B x (1 + R): -F / N before every step (NaN where that evaluation failed)
    n_bad_steps: np.ndarray  # B x (1 + R): steps at which the problem's evaluation reported info != 0 and its parameters were kept
    n_launches: int
    seed: int
    kernel: str = "rbf"
    jitter: float = 1e-6
    X: Optional[np.ndarray] = None   # nX x N x d
    Y: Optional[np.ndarray] = None   # B x N
    engine: object = None

    def model(self, b: int):
        """A ``SparseGPR`` over data set b that carries the fitted parameters (``posterior_predictive`` works as after ``train_model``)."""
        from .gp_shim import GaussianLikelihood, MaternKernel, RBFKernel
        from .models import SparseGPR
        if self.X is None or self.Y is None:
            raise ValueError("this result does not carry the data")
        d = self.theta.shape[1] - 2
        eng = self.engine if hasattr(self.engine, "suffstats") else None
        dev = eng.device if eng is not None else torch.device("cpu")
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
        base = RBFKernel(ard_num_dims=d) if self.kernel == "rbf" else MaternKernel(nu=1.5 if self.kernel == "matern32" else 2.5, ard_num_dims=d)
        m = SparseGPR(t(self.X[b if self.X.shape[0] > 1 else 0]), t(self.Y[b]), GaussianLikelihood(), t(self.Z[b]), engine=eng,
                      jitter=self.jitter, kernel=base)
        m.base_covar_module.base_kernel.lengthscale = t(self.theta[b, :d])
        m.base_covar_module.outputscale = float(self.theta[b, d])
        m.likelihood.noise = float(self.theta[b, d + 1])
        return m

    def predict(self, X_test, Y_test=None, pred_noise=True, probs=None):
        """The plug-in predictive at the fitted ``theta`` and ``Z`` of every data set (``sgpr_predict.SgprMixturePredictive`` with
        S = 1; theta is constrained already: no exp) -- ``Ml2Result.predict``'s counterpart."""
        if self.X is None or self.Y is None:
            raise ValueError("this result does not carry the data")
        from .sgpr_predict import predict_sgpr_theta_batch
        return predict_sgpr_theta_batch(self.X if self.X.shape[0] > 1 else self.X[0], self.Y, self.Z, self.theta[:, None, :], X_test,
                                        Y_test, kernel=self.kernel, jitter=self.jitter, pred_noise=pred_noise, engine=self.engine,
                                        probs=probs)

    def sample_nuts(self, n_samples: int, tune: int, chains: int = 1, seed=None, **opts):
        """NUTS over theta for every data set at its fitted Z -- the reference's ``train_fixed_model`` protocol (ML-II for Z, then NUTS
        over theta at that Z) for the B data sets at once (``sgpr_nuts.sample_sgpr_nuts_batch``: one device-resident batch of
        B x chains chains).  The best start's Z, the result's kernel and jitter; every chain starts at the log of the fitted theta,
        [log ls | log sqrt(sf2) | log sqrt(s2)].  ``opts`` go to ``sample_sgpr_nuts_batch`` (max_treedepth, step_scale, ...).
        Returns an ``SgprNutsResult``."""
        from .sgpr_nuts import sample_sgpr_nuts_batch
        if self.X is None or self.Y is None:
            raise ValueError("this result does not carry the data")
        d = self.theta.shape[1] - 2
        start = np.concatenate([np.log(self.theta[:, :d]), 0.5 * np.log(self.theta[:, d:])], 1)[:, None, :]
        opts.setdefault("start", np.broadcast_to(start, (self.theta.shape[0], int(chains), d + 2)))
        opts.setdefault("engine", self.engine)
        return sample_sgpr_nuts_batch(self.X if self.X.shape[0] > 1 else self.X[0], self.Y, self.Z, n_samples, tune, chains=chains,
                                      kernel=self.kernel, seed=seed, jitter=self.jitter, **opts)


def sgpr_start(X_b, Z_init_b, seed, b, r):
    """Start r of data set b: (raw [d + 2], Z [M x d]).  Start 0 is (0, Z_init); start r >= 1 draws raw ~ N(0, 1) and M distinct rows of
    the data set from a generator seeded by (seed, b, r)."""
    N, d = X_b.shape
    M = Z_init_b.shape[0]
    if r == 0:
        return np.zeros(d + 2), np.array(Z_init_b, dtype=np.float64)
    if M > N:
        raise ValueError("a restart draws its M = %d inducing inputs from the N = %d rows of the data set: M <= N" % (M, N))
    rng = np.random.default_rng([int(seed), int(b), int(r)])
    return rng.standard_normal(d + 2), X_b[rng.choice(N, M, replace=False)].copy()


def sgpr_theta(raw):
    """[ls | sf2 | s2] of the raw parameters, the parametrisation of ``SparseGPR``: softplus, the noise with its floor."""
    th = F.softplus(raw).contiguous()
    th[:, -1] = th[:, -1] + NOISE_FLOOR
    return th


def adam_step(par, grad, m, v, t, ok, lr, pow1, pow2):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) on the rows of ``par`` with ok[p]; the other rows, their moments and
    their step counts stay as they are.  t: int64 step counts per row; pow1 / pow2: beta^k for k = 0.. as host-computed tables on the
    device (the bias corrections are 1 - beta ** step, as the optimiser forms them).  In place."""
    b1, b2 = ADAM_BETAS
    okc = ok[:, None]
    g = torch.where(okc, grad, torch.zeros_like(grad))
    t_new = t + ok.to(t.dtype)
    m_new = torch.lerp(m, g, 1.0 - b1)
    v_new = (v * b2).addcmul_(g, g, value=1.0 - b2)
    bc1 = (1.0 - pow1[t_new])[:, None]
    bc2_sqrt = (1.0 - pow2[t_new]).sqrt()[:, None]
    denom = (v_new.sqrt() / bc2_sqrt).add_(ADAM_EPS)
    new = par - (lr / bc1) * (m_new / denom)
    par.copy_(torch.where(okc, new, par))
    m.copy_(torch.where(okc, m_new, m))
    v.copy_(torch.where(okc, v_new, v))
    t.copy_(t_new)


def fit_sgpr_batch(X, Y, Z_init, kernel="rbf", n_restarts=0, max_steps=2000, lr=0.01, learn_Z=True, jitter=1e-6, seed=None, engine=None):
    """Train B sparse GP regressions x (1 + n_restarts) starts in lock step: ``SparseGPR.train_model`` with Adam(lr) for every problem,
    one ``vfe_eval_batch`` launch per step (and one more for the final bounds).

    X: N x d (shared) or B x N x d; Y: B x N (or N); Z_init: M x d (shared) or B x M x d.  The parameters are ``SparseGPR``'s:
    lengthscales and outputscale are softplus of a raw parameter, the noise softplus + 1e-4, raw = 0 at start 0; the loss is -F / N.
    A problem whose evaluation reports ``info != 0`` at a step keeps its parameters and its optimiser state for that step; the step is
    counted in ``n_bad_steps``.  Returns an ``SgprBatchResult``."""
    _check_kernel(kernel)
    X = np.asarray(X, dtype=np.float64)
    X = X[None] if X.ndim == 2 else X
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y[None] if Y.ndim == 1 else Y
    Z_init = np.asarray(Z_init, dtype=np.float64)
    Z_init = Z_init[None] if Z_init.ndim == 2 else Z_init
    if X.ndim != 3 or Y.ndim != 2 or Z_init.ndim != 3:
        raise ValueError("X must be N x d or B x N x d, Y B x N, Z_init M x d or B x M x d (got %s, %s, %s)" % (X.shape, Y.shape, Z_init.shape))
    B = Y.shape[0]
    if X.shape[0] not in (1, B) or Z_init.shape[0] not in (1, B):
        raise ValueError("X holds %d data sets and Z_init %d inducing sets for %d targets" % (X.shape[0], Z_init.shape[0], B))
    _check_sparse_data(X[0], Y.shape[1], Z_init[0])
    if n_restarts < 0 or max_steps < 0:
        raise ValueError("n_restarts and max_steps must not be negative")
    N, d = X.shape[1:]
    M = Z_init.shape[1]
    R1 = 1 + int(n_restarts)
    P = B * R1
    seed = int(np.random.SeedSequence().generate_state(1)[0]) if seed is None else int(seed)
    raw0, Z0 = np.empty((P, d + 2)), np.empty((P, M, d))
    for b in range(B):
        for r in range(R1):
            raw0[b * R1 + r], Z0[b * R1 + r] = sgpr_start(X[b if X.shape[0] > 1 else 0], Z_init[b if Z_init.shape[0] > 1 else 0], seed, b, r)
    eng = _engine(engine)
    dev = eng.device
    Xd, Yd = _dev(X, eng), _dev(Y, eng)
    ix = torch.as_tensor(np.repeat(np.arange(B) if X.shape[0] > 1 else np.zeros(B, dtype=np.int64), R1).astype(np.int32), device=dev)
    iy = torch.as_tensor(np.repeat(np.arange(B), R1).astype(np.int32), device=dev)
    iz = torch.arange(P, dtype=torch.int32, device=dev)
    nh = d + 2
    par = torch.cat([_dev(raw0, eng), _dev(Z0.reshape(P, M * d), eng)], 1)   # P x (d + 2 + M d)
    m, v = torch.zeros_like(par), torch.zeros_like(par)
    t = torch.zeros(P, dtype=torch.int64, device=dev)
    pow1 = torch.as_tensor([ADAM_BETAS[0] ** k for k in range(max_steps + 1)], dtype=torch.float64, device=dev)
    pow2 = torch.as_tensor([ADAM_BETAS[1] ** k for k in range(max_steps + 1)], dtype=torch.float64, device=dev)
    losses = torch.full((max_steps, P), float("nan"), dtype=torch.float64, device=dev)
    n_bad = torch.zeros(P, dtype=torch.int64, device=dev)
    grad = torch.zeros_like(par)

    def evaluate(want_grad):
        theta = sgpr_theta(par[:, :nh])
        Zc = par[:, nh:].reshape(P, M, d).contiguous()
        return eng.vfe_eval_batch(Xd, Yd, Zc, theta, ix=ix, iy=iy, iz=iz, kernel=kernel, jitter=jitter, want_grad=want_grad,
                                  want_gz=want_grad and learn_Z)

    for step in range(max_steps):
        out, gz, info = evaluate(True)
        ok = info == 0
        losses[step] = -out[:, 0] / N
        n_bad += (~ok).to(n_bad.dtype)
        grad[:, :nh] = -out[:, 1:1 + nh] / N * torch.sigmoid(par[:, :nh])  # d softplus(raw) / d raw
        if learn_Z:
            grad[:, nh:] = -gz.reshape(P, M * d) / N
        adam_step(par, grad, m, v, t, ok, lr, pow1, pow2)
    out, _, info = evaluate(False)
    elbo_all = out[:, 0].cpu().numpy().reshape(B, R1)
    theta_all = sgpr_theta(par[:, :nh]).cpu().numpy().reshape(B, R1, nh)
    Z_all = par[:, nh:].cpu().numpy().reshape(B, R1, M, d)
    best = np.where(np.isnan(elbo_all), -np.inf, elbo_all).argmax(1)
    rows = np.arange(B)
    return SgprBatchResult(theta=theta_all[rows, best], Z=Z_all[rows, best], elbo=elbo_all[rows, best], best=best, theta_all=theta_all,
                           Z_all=Z_all, elbo_all=elbo_all, losses=losses.cpu().numpy().reshape(max_steps, B, R1),
                           n_bad_steps=n_bad.cpu().numpy().reshape(B, R1), n_launches=max_steps + 1, seed=seed, kernel=kernel,
                           jitter=float(jitter), X=X, Y=Y, engine=eng)
