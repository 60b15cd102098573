"""NUTS targets over ``[log ls_1..d, log sig_f, log sig_n]``: what ``hmc.sample_nuts`` / ``sample_nuts_device`` evaluate.

``HmcTarget`` (VFE bound, Z fixed), ``ExactHmcTarget`` (exact marginal likelihood) and ``JointHmcTarget`` (VFE bound, Z sampled)
share one density recipe -- PyMC3's log transform, its test point, the theta priors and the chain rule to the unconstrained
variables -- which lives here once, beside the two pieces every target over a ``CollapsedBound`` shares (``composite.
CompositeHmcTarget`` included): the single-launch evaluation and the test for the device-resident sampler.

``SgpmcTarget`` (GPflow's SGPMC: theta and the whitened inducing values, what ``hmc.sample_hmc`` evaluates) has GPflow's softplus
transforms and priors instead, and its own evaluation sequence over the whitened statistics.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .core import WHITENED_ROWS_MIN_WORK, CollapsedBound, SgpTimeoutError, device_run_fits, whitened_rows_layout

_LOG_2_OVER_PI = math.log(2.0) - math.log(math.pi)
_HALF_LOG_2PI = 0.9189385332046727


# ---------------------------------------------------------------------------------------------
# shared by every target
# ---------------------------------------------------------------------------------------------
def as_floats(q):
    """The position as plain floats, converted once (the sampler hands an ndarray)."""
    return q.tolist() if hasattr(q, "tolist") else [float(v) for v in q]


def in_range(theta):
    """exp() of the log-transformed variables must stay representable; beyond it the density is treated as zero (PyMC3:
    non-finite logp -> divergence), never an exception."""
    return all(math.isfinite(v) and abs(v) < 300.0 for v in theta)


def single_launch_ok(bound, M, want_gz=False):
    """The bound evaluates this shape in one launch (``CollapsedBound._small_ok``; a test double without one never does)."""
    return hasattr(bound, "_small_ok") and bound._small_ok(M, want_gz=want_gz)


def single_launch_eval(bound, Z, theta, n_grad, want_gz=False, composite=None):
    """ONE launch: transforms, priors, Jacobians and the chain rule are applied on the device (mode SGP_SMALL_HMC).
    Returns (logp, its first ``n_grad`` gradients, dF/dZ device tensor or None), or None where the factorisation failed."""
    h, info, gz = bound._small_eval(Z, theta, 1, True, want_gz, composite)
    bound.n_evals += 1
    bound.n_grads += 1
    hl = h.tolist()
    if info != 0 or not math.isfinite(hl[0]):
        return None
    return hl[0], hl[1:1 + n_grad], gz


def device_sampler_ok(bound, entry, M, want_gz=False, n_draws_total=None, max_treedepth=10):
    """True when ``hmc.sample_nuts_device`` can run a target over ``bound``: the engine has the persistent kernel ``entry``, the
    bound takes the single-launch path -- and, when the run length is given, its worst case (every tree at the depth limit)
    stays inside that kernel's cumulative int counters (``device_run_fits``); the host-driven sampler over the same single
    launch takes the longer runs."""
    ok = hasattr(bound.engine, entry) and single_launch_ok(bound, M, want_gz)
    return ok and (n_draws_total is None or device_run_fits(int(bound.X.shape[0]), n_draws_total, max_treedepth))


# ---------------------------------------------------------------------------------------------
# the [log ls, log sig_f, log sig_n] head: ls ~ Gamma(2, 1), sig_f ~ HalfCauchy(1), sig_n ~ HalfCauchy(1)
# ---------------------------------------------------------------------------------------------
def theta_prior(ls, sf, sn):
    """(log prior, d/d ls list, d/d sig_f, d/d sig_n) in the constrained variables."""
    lp = sum(math.log(v) - v for v in ls)
    g_ls = [1.0 / v - 1.0 for v in ls]
    lp += (_LOG_2_OVER_PI - math.log1p(sf * sf)) + (_LOG_2_OVER_PI - math.log1p(sn * sn))
    return lp, g_ls, -2.0 * sf / (1.0 + sf * sf), -2.0 * sn / (1.0 + sn * sn)


def theta_logp_and_grad(theta, ls, sf, sn, F, g_ls=None, g_sf2=None, g_s2=None, finite_grad=False):
    """F(ls, sf^2, sn^2) and its gradients -> (logp, grad) in the unconstrained theta: + priors + log-Jacobians sum(theta);
    d/d log v = v d/d v, + 1 from the Jacobian.  ``g_ls=None``: the value alone, (logp, None).  ``finite_grad``: a non-finite
    gradient entry gives (-inf, zeros)."""
    lp, pg_ls, pg_sf, pg_sn = theta_prior(ls, sf, sn)
    logp = F + lp + sum(theta)
    if g_ls is None:
        return logp, None
    grad = [ls[j] * (g_ls[j] + pg_ls[j]) + 1.0 for j in range(len(ls))]
    grad.append(sf * (2.0 * sf * g_sf2 + pg_sf) + 1.0)
    grad.append(sn * (2.0 * sn * g_s2 + pg_sn) + 1.0)
    if finite_grad and not all(math.isfinite(v) for v in grad):
        return -math.inf, [0.0] * len(grad)
    return logp, grad


class _LogThetaTarget:
    """``start`` / ``constrain`` of a target whose position begins with the d + 2 log-transformed hyper-parameters."""

    d: int

    def start(self):
        """PyMC3's test point in the unconstrained space: Gamma(2,1) -> mean 2, HalfCauchy(1) -> 1."""
        return [math.log(2.0)] * self.d + [0.0, 0.0]

    def constrain(self, theta):
        th = [float(v) for v in theta]
        return {"ls": [math.exp(v) for v in th[: self.d]], "sig_f": math.exp(th[self.d]), "sig_n": math.exp(th[self.d + 1])}


# ---------------------------------------------------------------------------------------------
# HMC target: VFE logp + priors + log-Jacobians  (reference models/bayesian_sgpr_hmc.py:60-71)
# ---------------------------------------------------------------------------------------------
class HmcTarget(_LogThetaTarget):
    """logp(theta_unc) and its gradient, theta_unc = [log ls_1..d, log sig_f, log sig_n].

    ls ~ Gamma(alpha=2, beta=1), sig_f ~ HalfCauchy(1), sig_n ~ HalfCauchy(1), all log-transformed
    as PyMC3 does for positive variables; covariance sig_f**2 * ExpQuad(ls), noise sig_n, Kuu jitter
    1e-6 (``stabilize``).  A failed Cholesky gives logp = -inf (PyMC3: ``on_error='nan'``), which the
    sampler treats as a divergence, never an exception.
    """

    def __init__(self, bound: CollapsedBound, Z, gradient="parity"):
        """gradient: "parity" (default) -- every gradient holds 1e-6 against the CPU path (north_star): where the streaming order's error
        estimate is beyond 3 x its tolerance a leapfrog runs in the whitened order (74 instead of 49 ms at C5).
        "sampler" -- opt-in for NUTS in such a region: the extended order serves value AND gradient as far as its VALUE holds (2^14 x the
        tolerance; 55 ms per leapfrog at C5).  The energy still meets 1e-8 per datum; the force is the extended order's explicit-Phibar
        gradient, off by up to ~1e-4 relative at the far end of that range (profiles/r04_extended_order_c5.jsonl) -- but a deterministic
        function of theta: the tier of every evaluation is the one its OWN error estimate names (`strict`), never the guard's memory of
        earlier evaluations.  Leapfrog with a deterministic approximate force is still volume preserving and reversible, and the
        accept step uses the accurate energy, so the chain still targets the exact posterior (tests/test_posterior_pin.py holds the
        mode to the same 4 MCSE pin as the default); only the acceptance rate pays for the force error."""
        if gradient not in ("parity", "sampler"):
            raise ValueError("gradient must be 'parity' or 'sampler'")
        self.bound = bound
        self.Z = bound._prep_Z(Z)
        self.d = bound.d
        self.ndim = self.d + 2
        self.gradient = gradient

    def device_sampler_ok(self, n_draws_total=None, max_treedepth=10):
        """True when ``hmc.sample_nuts_device`` can run this target (``sgp_small_nuts``; see ``targets.device_sampler_ok``)."""
        return device_sampler_ok(self.bound, "small_nuts", self.Z.shape[0], False, n_draws_total, max_treedepth)

    def run_on_device(self, q0, tune, n_samples, rng_state, **sampler_opts):
        b = self.bound
        return b.engine.small_nuts(b.X, b.y, self.Z, q0, tune, n_samples, rng_state, jitter=b.jitter, kernel=b.kernel, **sampler_opts)

    def logp(self, theta):
        theta = as_floats(theta)
        if not in_range(theta):
            return -math.inf
        if single_launch_ok(self.bound, self.Z.shape[0]):
            return self.logp_and_grad(theta)[0]
        p = self.constrain(theta)  # the value alone: no gradient pass
        F, parts = self.bound.value(self.Z, p["ls"], p["sig_f"] ** 2, p["sig_n"] ** 2, raise_on_fail=False,
                                    **({"strict": True} if self.gradient == "sampler" else {}))
        if parts.get("info", 0) != 0 or not math.isfinite(F):
            return -math.inf
        return theta_logp_and_grad(theta, p["ls"], p["sig_f"], p["sig_n"], F)[0]

    def logp_and_grad(self, theta):
        """Returns (logp, grad list[d+2]).  One call = one HMC leapfrog's worth of device work."""
        theta = as_floats(theta)
        bad = (-math.inf, [0.0] * self.ndim)
        if not in_range(theta):
            return bad
        b = self.bound
        if single_launch_ok(b, self.Z.shape[0]):
            r = single_launch_eval(b, self.Z, theta, self.ndim)
            return bad if r is None else r[:2]
        p = self.constrain(theta)
        ls, sf, sn = p["ls"], p["sig_f"], p["sig_n"]
        kw = {"grad_reach": b.extended_range, "strict": True} if self.gradient == "sampler" else {}
        F, g = b.value_and_grad(self.Z, ls, sf * sf, sn * sn, want_gz=False, raise_on_fail=False, **kw)
        if g.get("info", 0) != 0 or not math.isfinite(F):
            return bad
        # (one conversion of g["ls"]: indexing a tensor element by element costs ~1.5 us each -- 27 us per leapfrog at d = 18)
        return theta_logp_and_grad(theta, ls, sf, sn, F, g["ls"].tolist(), g["sf2"], g["s2"])


# ---------------------------------------------------------------------------------------------
# exact-GP HMC target  (reference models/gpr_hmc.py:43-59)
# ---------------------------------------------------------------------------------------------
EXACT_MAX_N = 4096  # SGP_MAX_INDUCING: the largest N sgp_exact_eval factors


class ExactHmcTarget(_LogThetaTarget):
    """logp(theta_unc) and its gradient for NUTS over the EXACT GP marginal likelihood, theta_unc = [log ls_1..d, log sig_f, log sig_n].

    ``pm.gp.Marginal(cov_func=sig_f**2 * ExpQuad(ls)).marginal_likelihood(y, X, noise=sig_n)`` with ls ~ Gamma(2, 1), sig_f ~
    HalfCauchy(1), sig_n ~ HalfCauchy(1), log-transformed: the density is log N(y | 0, K + (sig_n^2 + jitter) I) plus
    ``HmcTarget``'s priors and log-Jacobians.  ``jitter`` defaults to 0: Marginal adds only WhiteNoise(sig_n) to the diagonal.
    One ``logp_and_grad`` is one ``engine.exact_eval`` (include/sgp.h: sgp_exact_eval) and one device-to-host copy.  A non-zero
    status word (A numerically not positive definite, the conditioning gate), a non-finite F or a non-finite gradient entry gives
    (-inf, zeros), which the sampler treats as a divergence; it never raises.  Single process: the target makes no collectives
    (N <= 4096 fits one device)."""

    def __init__(self, X, y, kernel="rbf", engine=None, jitter=0.0):
        if engine is None:
            from .engine import HipEngine
            engine = HipEngine(X.device if X.is_cuda else None)
        if kernel not in ("rbf", "matern32", "matern52"):
            raise ValueError("ExactHmcTarget takes 'rbf', 'matern32' or 'matern52' (got %r)" % (kernel,))
        self.engine = engine
        if X.dim() == 1:
            X = X[:, None]
        self.X = X.to(dtype=torch.float64, device=engine.device).contiguous()
        self.y = y.to(dtype=torch.float64, device=engine.device).reshape(-1).contiguous()
        if self.X.shape[0] != self.y.shape[0]:
            raise ValueError("X has %d rows, y has %d" % (self.X.shape[0], self.y.shape[0]))
        if self.X.shape[0] > EXACT_MAX_N:
            raise ValueError("the exact GP takes at most N = %d training rows (got %d)" % (EXACT_MAX_N, self.X.shape[0]))
        self.kernel = kernel
        self.jitter = float(jitter)
        self.d = int(self.X.shape[1])
        self.ndim = self.d + 2
        self.n_evals = 0

    def _eval(self, theta, want_grad):
        """(logp, grad or None) at theta."""
        theta = as_floats(theta)
        bad = (-math.inf, [0.0] * self.ndim if want_grad else None)
        if not in_range(theta):
            return bad
        p = self.constrain(theta)
        ls, sf, sn = p["ls"], p["sig_f"], p["sig_n"]
        self.n_evals += 1
        r = self.engine.exact_eval(self.X, self.y, ls, sf * sf, sn * sn + self.jitter, kernel=self.kernel, want_grad=want_grad)
        if r["info"] != 0 or not math.isfinite(r["F"]):
            return bad
        if not want_grad:
            return theta_logp_and_grad(theta, ls, sf, sn, r["F"])
        return theta_logp_and_grad(theta, ls, sf, sn, r["F"], r["ls"], r["sf2"], r["s2"], finite_grad=True)

    def logp(self, theta):
        return self._eval(theta, False)[0]

    def logp_and_grad(self, theta):
        """Returns (logp, grad list[d+2])."""
        return self._eval(theta, True)


# ---------------------------------------------------------------------------------------------
# joint HMC target: theta AND the inducing inputs  (reference models/all_in_HMC.py:45-61)
# ---------------------------------------------------------------------------------------------
class JointHmcTarget(_LogThetaTarget):
    """logp(q) and its gradient for NUTS over the hyper-parameters and the inducing inputs together,
    q = [log ls_1..d, log sig_f, log sig_n, vec(Z)] with Z row-major M x d, untransformed (ndim = d + 2 + M d).

    The same VFE ``MarginalSparse`` density and theta priors / Jacobians as ``HmcTarget``, plus Z ~ Normal(0, 1)
    elementwise with its normalising constants, so ``logp`` is PyMC3's model logp.  Kuu jitter 1e-6 (``stabilize``).
    A value of theta outside the representable range or a failed factorisation gives -inf, never an exception."""

    def __init__(self, bound: CollapsedBound, M: int):
        if bound.kernel == "composite":
            raise ValueError("the joint target takes stationary kernels (no dF/dZ for composite kernels)")
        self.bound = bound
        self.d = bound.d
        self.M = int(M)
        self.ndim = self.d + 2 + self.M * self.d

    def start(self):
        """PyMC3's test point: HmcTarget's for theta, the prior mean 0 for Z."""
        return super().start() + [0.0] * (self.M * self.d)

    def device_sampler_ok(self, n_draws_total=None, max_treedepth=10):
        """True when ``hmc.sample_nuts_device`` can run this target (``sgp_small_nuts_joint``: the single-launch class with dF/dZ;
        see ``targets.device_sampler_ok``)."""
        return device_sampler_ok(self.bound, "small_nuts_joint", self.M, True, n_draws_total, max_treedepth)

    def run_on_device(self, q0, tune, n_samples, rng_state, **sampler_opts):
        b = self.bound  # (Z is part of the position)
        return b.engine.small_nuts_joint(b.X, b.y, self.M, q0, tune, n_samples, rng_state, jitter=b.jitter, kernel=b.kernel, **sampler_opts)

    def _split(self, q):
        q = as_floats(q)
        return q[:self.d + 2], q[self.d + 2:]

    def constrain(self, q):
        th, z = self._split(q)
        return dict(super().constrain(th), Z=np.asarray(z, dtype=np.float64).reshape(self.M, self.d))

    def logp(self, q):
        return self.logp_and_grad(q)[0]

    def logp_and_grad(self, q):
        """Returns (logp, grad list[ndim]).  One call = one leapfrog's evaluation, dF/dZ included."""
        th, z = self._split(q)
        bad = (-math.inf, [0.0] * self.ndim)
        if not in_range(th) or not all(math.isfinite(v) for v in z):
            return bad
        b = self.bound
        zz = np.asarray(z, dtype=np.float64)
        Zt = torch.from_numpy(zz.reshape(self.M, self.d)).to(b.engine.device)
        zprior = -0.5 * float(zz @ zz) - _HALF_LOG_2PI * zz.size
        if single_launch_ok(b, self.M, want_gz=True):
            r = single_launch_eval(b, Zt, th, self.d + 2, want_gz=True)
            if r is None:
                return bad
            logp, grad, gz = r
        else:
            p = super().constrain(th)
            ls, sf, sn = p["ls"], p["sig_f"], p["sig_n"]
            F, g = b.value_and_grad(Zt, ls, sf * sf, sn * sn, want_gz=True, raise_on_fail=False)
            if g.get("info", 0) != 0 or not math.isfinite(F):
                return bad
            logp, grad = theta_logp_and_grad(th, ls, sf, sn, F, g["ls"].tolist(), g["sf2"], g["s2"])
            gz = g["Z"]
        return logp + zprior, grad + (gz.detach().to("cpu").numpy().reshape(-1) - zz).tolist()


# ---------------------------------------------------------------------------------------------
# SGPMC target: theta AND the whitened inducing values  (reference models/sgp_hmc.py:36-49; Hensman et al. 2015)
# ---------------------------------------------------------------------------------------------
_SGPMC_NOISE_FLOOR = 1e-6


def _softplus(x):
    return x + math.log1p(math.exp(-x)) if x > 0.0 else math.log1p(math.exp(x))


def _sigmoid(x):
    if x >= 0.0:
        return 1.0 / (1.0 + math.exp(-x))
    t = math.exp(x)
    return t / (1.0 + t)


def _softplus_inv(c):
    return c + math.log(-math.expm1(-c))


def multiclass_labels(y, num_classes=None):
    """The class count C of a label vector for the robust-max likelihood: the labels must be integers 0 .. C-1, C = max + 1 unless
    ``num_classes`` says more (a class may have no datum); 2 <= C <= 16 (SGP_MAX_CLASSES).  Anything else raises ValueError."""
    yh = torch.as_tensor(y).detach().to("cpu", torch.float64).reshape(-1)
    if yh.numel() == 0 and num_classes is None:
        raise ValueError("no labels and no num_classes: the class count cannot be inferred")
    if yh.numel() and not bool((torch.isfinite(yh) & (yh >= 0.0) & (yh == torch.floor(yh))).all()):
        raise ValueError("multi-class labels must be the integers 0 .. C-1")
    top = int(yh.max()) + 1 if yh.numel() else 0
    C = top if num_classes is None else int(num_classes)
    if num_classes is not None and (C != num_classes or C < top):
        raise ValueError("num_classes = %r does not hold the labels 0 .. %d" % (num_classes, top - 1))
    if not 2 <= C <= 16:
        raise ValueError("the class count must be 2 .. 16 (got %d)" % C)
    return C


class SgpmcTargetBase:
    """What the SGPMC targets share outside an evaluation (``SgpmcTarget`` here, ``composite.CompositeSgpmcTarget``): the data intake
    with the label rules, ``set_Z`` and the caller-owned T.  A target sets ``_NAME`` (its name in the intake's error text) and
    ``n_theta`` ahead of ``set_Z``.  The evaluations themselves stay with the targets: sharing their envelope through hooks cost
    2 - 3 us of calls per evaluation, 1 % at the small shapes."""

    LIKELIHOODS = ("gaussian", "bernoulli", "bernoulli_logit", "poisson", "multiclass")
    n_latent = 1   # latent GPs = columns of whitened inducing values

    def _intake(self, X, y, likelihood, engine):
        """Sets engine, X (N x d), y (N, on the device, Bernoulli labels as {-1, +1}), likelihood, N, d; returns y on the host."""
        if likelihood not in self.LIKELIHOODS:
            raise ValueError("%s takes the likelihoods %s (got %r)" % (self._NAME, ", ".join(self.LIKELIHOODS), likelihood))
        if engine is None:
            from .engine import HipEngine
            engine = HipEngine(X.device if X.is_cuda else None)
        self.engine = engine
        if X.dim() == 1:
            X = X[:, None]
        self.X = X.to(dtype=torch.float64, device=engine.device).contiguous()
        yh = y.detach().to(dtype=torch.float64, device="cpu").reshape(-1)
        if self.X.shape[0] != yh.shape[0]:
            raise ValueError("X has %d rows, y has %d" % (self.X.shape[0], yh.shape[0]))
        if likelihood in ("bernoulli", "bernoulli_logit"):   # {0, 1} or {-1, +1} labels -> {-1, +1}, on the host
            if not bool(((yh == 0.0) | (yh == 1.0) | (yh == -1.0)).all()) or (bool((yh == 0.0).any()) and bool((yh == -1.0).any())):
                raise ValueError("Bernoulli labels must be {0, 1} or {-1, +1}")
            if bool((yh == 0.0).any()):
                yh = 2.0 * yh - 1.0
        elif likelihood == "poisson" and not bool((torch.isfinite(yh) & (yh >= 0.0) & (yh == torch.floor(yh))).all()):
            raise ValueError("Poisson counts must be non-negative integers")
        self.y = yh.to(engine.device).contiguous()
        self.likelihood = likelihood
        self.N, self.d = int(self.X.shape[0]), int(self.X.shape[1])
        self.n_evals = 0
        self._t_keep = None
        return yh

    def set_Z(self, Z):
        if Z.dim() == 1:
            Z = Z[:, None]
        Z = Z.detach().to(dtype=torch.float64, device=self.engine.device).contiguous()
        if Z.shape[1] != self.d:
            raise ValueError("Z has %d columns, X has %d" % (Z.shape[1], self.d))
        self.Z = Z
        self.M = int(Z.shape[0])
        self.ndim = self.n_theta + self.M * self.n_latent

    def _t_for(self):
        e = self.engine
        if not hasattr(e, "kfu_buffer"):
            return None
        need = ((max(self.N, 1) + 255) // 256 * 256) * ((self.M + 127) // 128 * 128)
        if self._t_keep is None or self._t_keep.numel() < need:
            self._t_keep = e.kfu_buffer(self.N, self.M)
        return self._t_keep


class SgpmcTarget(SgpmcTargetBase):
    """logp(q) and its gradient for HMC over the hyper-parameters and the whitened inducing values together (GPflow's ``SGPMC``, with a
    Gaussian likelihood models/sgp_hmc.py:38-43), q = [x_var | x_ls (d) | x_noise | v (M)] unconstrained, ndim = d + 2 + M.

    kernel variance = softplus(x_var), lengthscales = softplus(x_ls), noise variance = 1e-6 + softplus(x_noise); Gamma(2, 1) on each
    of the three evaluated at the constrained value plus log sigmoid(x) for the transform (models/sgp_hmc.py:47-49); v ~ N(0, I); K_uu
    jitter 1e-5 (models/sgp_hmc.py:20).  [UPSTREAM] the transforms (softplus, the 1e-6 floor of the likelihood variance) and the prior
    convention are GPflow's published behaviour as recalled: GPflow is not installed here and nothing was checked against it.

    The density F(v, theta) is stated in include/sgp.h (sgp_sgpmc_from_whitened_stats).  One evaluation is ``kuu`` -> ``kuu_factor`` ->
    ``suffstats_whitened`` (``suffstats_whitened_rows`` where ``core.whitened_rows_layout`` says so, T kept for pass 2) -> ``sgpmc_tail``
    -> ``suffstats_bwd_factored`` -> ``kuu_bwd``, one result buffer and one device-to-host copy; transforms, priors and the chain rule to
    x run on the host.  A non-zero ``kuu_factor`` status or a non-finite value gives (-inf, zeros), never an exception (a device
    time-out still raises ``SgpTimeoutError``).  Stationary kernels, one process.  Z is fixed per evaluation and may be replaced
    between evaluations (``set_Z``: the warm-up of ``sgp_hmc.train_sgp_hmc`` optimises it).

    ``likelihood``: "gaussian" (the above), or one of the non-conjugate likelihoods SGPMC exists for -- "bernoulli" (probit link),
    "bernoulli_logit" (labels {0, 1} or {-1, +1}) and "poisson" (log link, non-negative integer counts).  [UPSTREAM] GPflow's
    ``SGPMC.log_likelihood_lower_bound`` as recalled: ``conditional(..., q_sqrt=None, white=True)`` then
    ``likelihood.variational_expectations``.  They have no noise entry: q = [x_var | x_ls (d) | v (M)], ndim = d + 1 + M, the priors
    and transforms of the remaining entries unchanged.  One evaluation is ``kuu`` -> ``kuu_factor`` -> ``sgpmc_lik_rows`` ->
    ``sgpmc_lik_tail`` -> ``suffstats_bwd_factored(t_in = diag(dv) T, y = dmu, Cw = -2 I, s2 = 1, bbar = L^-T v)`` -> ``kuu_bwd``
    (include/sgp.h states the density, its adjoints and why pass 2 needs no new kernel), again with one device-to-host copy: the
    diagonal term of dF/d variance, sum_n dv_n, comes back in that copy and is added on the host, where pass 2's ``kappabar`` argument
    would have needed it before the launch.

    ``likelihood="multiclass"``: the robust-max likelihood over ``num_classes`` = C latent GPs that share the kernel and Z (labels are
    the integers 0 .. C-1; C = max + 1 when ``num_classes`` is None; 2 <= C <= 16), with ``robustmax_eps`` the probability mass spread
    over the wrong classes.  q = [x_var | x_ls (d) | vec(V) class-major], ndim = d + 1 + M C, ``constrain()["V"]`` is (C, M); priors
    and transforms of the theta entries unchanged.  One evaluation is ``kuu`` -> ``kuu_factor`` -> ``sgpmc_mc_rows`` ->
    ``sgpmc_mc_tail`` -> ``suffstats_bwd_factored(t_in = diag(dv) T - DMU V^T / (2 sf2), y = 0, Cw = -2 I, s2 = 1, bbar = 0)`` ->
    ``kuu_bwd``: ONE pass 2 whatever C is (include/sgp.h, the sgp_sgpmc_mc_rows section), one device-to-host copy."""

    _NAME = "SgpmcTarget"

    def __init__(self, X, y, Z, kernel="rbf", jitter=1e-5, engine=None, group=None, likelihood="gaussian", num_classes=None,
                 robustmax_eps=1e-3):
        from .core import _world
        if kernel not in ("rbf", "matern32", "matern52"):
            raise ValueError("SgpmcTarget takes the stationary kernels 'rbf', 'matern32', 'matern52' (got %r): composite kernels are "
                             "not supported" % (kernel,))
        if _world(group) > 1:
            raise ValueError("SgpmcTarget runs in one process: a group of %d ranks is not supported" % _world(group))
        yh = self._intake(X, y, likelihood, engine)
        self.eps = float(robustmax_eps)
        if likelihood == "multiclass":
            self.n_latent = self.num_classes = multiclass_labels(yh, num_classes)
            if not 0.0 < self.eps < 1.0:
                raise ValueError("robustmax_eps must lie in (0, 1) (got %r)" % (robustmax_eps,))
        elif num_classes is not None:
            raise ValueError("num_classes belongs to likelihood='multiclass' (got likelihood=%r)" % (likelihood,))
        self.n_theta = self.d + (2 if likelihood == "gaussian" else 1)   # [x_var | x_ls (d) | x_noise (Gaussian only)]
        self.kernel = kernel
        self.jitter = float(jitter)
        self._cw_keep = None
        self.whitened_rows_min_work = WHITENED_ROWS_MIN_WORK
        self.last_pass1 = None   # "suffstats_whitened" / "suffstats_whitened_rows": which pass 1 the last evaluation ran
        self.set_Z(Z)

    def start(self):
        """GPflow's defaults as the reference sets them (models/sgp_hmc.py:36): variance log(2)^2, lengthscales log 2, likelihood
        variance 1, v = 0."""
        ln2 = math.log(2.0)
        noise = [_softplus_inv(1.0 - _SGPMC_NOISE_FLOOR)] if self.likelihood == "gaussian" else []
        return [_softplus_inv(ln2 * ln2)] + [_softplus_inv(ln2)] * self.d + noise + [0.0] * (self.M * self.n_latent)

    def constrain(self, q):
        """The constrained values of a position; ``noise_variance`` only with the Gaussian likelihood."""
        x = as_floats(q)
        d = self.d
        c = {"variance": _softplus(x[0]), "lengthscales": [_softplus(t) for t in x[1:1 + d]]}
        if self.likelihood == "gaussian":
            c["noise_variance"] = _SGPMC_NOISE_FLOOR + _softplus(x[1 + d])
        c["V"] = np.asarray(x[self.n_theta:], dtype=np.float64)
        if self.likelihood == "multiclass":
            c["V"] = c["V"].reshape(self.num_classes, self.M)   # class-major
        return c

    def _cw(self):
        """-2 I (M x M): the whitened core that turns the factored pass 2 into the N-side gradient of a non-conjugate likelihood."""
        if self._cw_keep is None or self._cw_keep.shape[0] != self.M:
            self._cw_keep = (-2.0 * torch.eye(self.M, dtype=torch.float64)).to(self.engine.device).contiguous()
        return self._cw_keep

    def _chain_gaussian(self, ls, sf2, s2, v, linv, result, vbar_kw, g, want_grad, want_gz):
        """Pass 1 over the whitened statistics, the Gaussian tail and (``want_grad``) the factored pass 2 into ``g``; returns Kuubar."""
        e, Z = self.engine, self.Z
        t_keep = None
        if whitened_rows_layout(e, self.kernel, self.N, self.M, self.whitened_rows_min_work):
            t_keep = self._t_for() if want_grad else None
            packed = e.suffstats_whitened_rows(self.X, self.y, Z, ls, sf2, linv, self.kernel, t_out=t_keep)
            self.last_pass1 = "suffstats_whitened_rows"
        else:
            packed = e.suffstats_whitened(self.X, self.y, Z, ls, sf2, linv, self.kernel)
            self.last_pass1 = "suffstats_whitened"
        res = e.sgpmc_tail(packed, v, s2, self.N, linv, with_adjoints=want_grad, result=result, **vbar_kw)
        if not want_grad:
            return None
        e.suffstats_bwd_factored(self.X, self.y, Z, ls, sf2, linv, res["Cw"], s2, res["bbar"], -1.0 / (2.0 * s2), self.kernel,
                                 want_gz=want_gz, out=g, **({"t_in": t_keep} if t_keep is not None else {}))
        return res["Kuubar"]

    def _chain_lik(self, ls, sf2, s2, v, linv, result, vbar_kw, g, want_grad, want_gz):
        """The same for a non-conjugate likelihood: the row pass over T, its tail, and pass 2 on T_in = diag(dv) T with y := dmu,
        Cw := -2 I, s2 := 1, bbar := L^-T v (kappabar = 0: sum_n dv_n is added on the host, see ``_eval``)."""
        e, Z = self.engine, self.Z
        t_keep = self._t_for()
        rows = e.sgpmc_lik_rows(self.X, self.y, Z, ls, sf2, 1.0, v, linv, t_keep, self.kernel, self.likelihood, want_adjoints=want_grad)
        self.last_pass1 = "sgpmc_lik_rows"
        res = e.sgpmc_lik_tail(rows, v, self.N, linv, with_adjoints=want_grad, result=result, **vbar_kw)
        if not want_grad:
            return None
        e.suffstats_bwd_factored(self.X, rows["dmu"], Z, ls, sf2, linv, self._cw(), 1.0, res["bbar"], 0.0, self.kernel,
                                 want_gz=want_gz, out=g, t_in=t_keep)
        return res["Kuubar"]

    def _zeros(self, n):
        z = self.__dict__.get("_zeros_keep")
        if z is None or z.numel() < n:
            z = self._zeros_keep = torch.zeros(max(n, 1), dtype=torch.float64, device=self.engine.device)
        return z[:n]

    def _chain_mc(self, ls, sf2, s2, v, linv, result, vbar_kw, g, want_grad, want_gz):
        """The same for the multi-class robust-max likelihood: V is C x M, and ONE pass 2 takes the N-side gradient of all classes from
        the folded T_in = diag(dv) T - DMU V^T / (2 sf2) the row pass leaves, with y := 0, bbar := 0, Cw := -2 I, s2 := 1."""
        e, Z = self.engine, self.Z
        t_keep = self._t_for()
        V = v.view(self.num_classes, self.M)
        rows = e.sgpmc_mc_rows(self.X, self.y, Z, ls, sf2, V, linv, t_keep, self.kernel, self.eps, want_adjoints=want_grad)
        self.last_pass1 = "sgpmc_mc_rows"
        res = e.sgpmc_mc_tail(rows, V, self.N, linv, with_adjoints=want_grad, result=result, **vbar_kw)
        if not want_grad:
            return None
        e.suffstats_bwd_factored(self.X, self._zeros(self.N), Z, ls, sf2, linv, self._cw(), 1.0, self._zeros(self.M), 0.0, self.kernel,
                                 want_gz=want_gz, out=g, t_in=t_keep)
        return res["Kuubar"]

    def _eval(self, q, want_grad, want_gz=False):
        x = as_floats(q)
        d, M, e, nt = self.d, self.M, self.engine, self.n_theta
        gaussian = self.likelihood == "gaussian"
        if len(x) != self.ndim:
            raise ValueError("the position has %d entries, expected %d theta + %d inducing values = %d" % (len(x), nt, self.ndim - nt,
                                                                                                         self.ndim))
        bad = (-math.inf, [0.0] * self.ndim if want_grad else None, None)
        if not all(math.isfinite(t) for t in x) or not all(abs(t) < 700.0 for t in x[:nt]):
            return bad
        sf2, ls = _softplus(x[0]), [_softplus(t) for t in x[1:1 + d]]
        s2 = _SGPMC_NOISE_FLOOR + _softplus(x[1 + d]) if gaussian else None
        if not (sf2 > 0.0 and all(t > 0.0 for t in ls)):   # softplus underflowed: outside the representable range
            return bad
        if not gaussian and self._t_for() is None:
            raise ValueError("the engine has no kfu_buffer: SgpmcTarget(likelihood=%r) needs the caller-owned T" % (self.likelihood,))
        self.n_evals += 1
        ng = d + 1 + (M * d if want_gz else 0)
        nv = M * self.n_latent
        extra = ng + nv if want_grad else 0
        result = e.result_buffer(extra)
        buf = result[0]
        head = buf.numel() - extra
        Kuu = e.kuu(self.Z, ls, sf2, self.jitter, self.kernel)
        linv, _ = e.kuu_factor(Kuu, info=result[2])   # the evaluation's status word is the K_uu status: the tails factor nothing
        v = torch.tensor(x[nt:], dtype=torch.float64).to(e.device)
        g = buf[head:head + ng] if want_grad else None
        chain = self._chain_gaussian if gaussian else (self._chain_mc if self.likelihood == "multiclass" else self._chain_lik)
        Kuubar = chain(ls, sf2, s2, v, linv, result, {"vbar_out": buf[head + ng:]} if want_grad else {}, g, want_grad, want_gz)
        if want_grad:
            e.kuu_bwd(self.Z, ls, sf2, Kuubar, g, self.kernel, want_gz=want_gz)
        host = buf.detach().to("cpu")   # the one host round trip
        o, info = e.read_result(host)
        if info < 0:
            raise SgpTimeoutError()
        F = float(o[0])
        if info != 0 or not math.isfinite(F):
            return bad
        # priors at the constrained values + log sigmoid(x) for the transform
        cons = [sf2] + ls + ([s2] if gaussian else [])
        sig = [_sigmoid(t) for t in x[:nt]]
        if not all(s > 0.0 for s in sig):
            return bad
        logp = F + sum(math.log(c) - c for c in cons) + sum(math.log(s) for s in sig)
        if not want_grad:
            return logp, None, None
        hl = host.tolist()
        gh = hl[head:head + d + 1]
        # dF/d variance, dF/d lengthscales and, Gaussian, dF/d s2 (SGP_SGPMC_OUT_S2BAR).  Non-conjugate: + sum_n dv_n = N out[4] on
        # dF/d variance (k(x_n, x_n) = variance), which pass 2's host scalar kappabar could not carry without a second host copy
        dF = [gh[d]] + gh[:d] + [float(o[3])] if gaussian else [gh[d] + float(o[4]) * self.N] + gh[:d]
        grad = [(dF[k] + 1.0 / cons[k] - 1.0) * sig[k] + (1.0 - sig[k]) for k in range(nt)] + hl[head + ng:head + ng + nv]
        if not all(math.isfinite(t) for t in grad):
            return bad
        gz = buf[head + d + 1:head + ng].reshape(M, d) if want_gz else None
        return logp, grad, gz

    def logp(self, q):
        return self._eval(q, False)[0]

    def logp_and_grad(self, q, want_gz=False):
        """(logp, grad list[ndim]); with ``want_gz`` (the warm-up over Z as well) also dlogp/dZ, an M x d tensor on the engine's
        device (None where the density is zero)."""
        r = self._eval(q, True, want_gz)
        return r if want_gz else r[:2]
