"""Sum-of-products covariance functions on the HIP core.

The reference's CO2 workload builds its covariance twice -- GPyTorch kernels for the optimisation stage
(experiments/co2_bayesian_sgpr_hmc.py:74-83) and PyMC3 ``pm.gp.cov`` objects for the NUTS stage (:107-149):

    n_per**2 * Periodic(1, period=1, ls=l_psmooth) * ExpQuad(1, l_pdecay)  +  n_med**2 * RatQuad(1, l_med, alpha)
      +  n_trend**2 * ExpQuad(1, l_trend)  +  n_noise**2 * Matern32(1, l_noise)

``CompositeKernel`` describes such a kernel as data (terms of amplitude * factors) and packs it into the parameter
block ``include/sgp.h`` documents (SGP_KERNEL_COMPOSITE); ``CollapsedBound(kernel="composite")`` evaluates the same
collapsed bound, its gradient with respect to every entry of the block, Z and the noise, and the predictive.
``CompositeHmcTarget`` is the NUTS target of the reference's PyMC3 model: Normal priors on the log-parameters,
HalfNormal(1) on the noise standard deviation.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import COMP_LEN
from .core import CollapsedBound, SgpTimeoutError, few_host_threads
from .hmc import next_seed, sample_nuts, sample_nuts_device, trace_summary
from .targets import (_SGPMC_NOISE_FLOOR, SgpmcTargetBase, _sigmoid, _softplus, _softplus_inv, as_floats, device_sampler_ok, in_range,
                      single_launch_eval, single_launch_ok)

EXPQUAD, MATERN32, MATERN52, RATQUAD, PERIODIC = 0, 1, 2, 3, 4
_FACTOR_IDS = {"expquad": EXPQUAD, "rbf": EXPQUAD, "matern32": MATERN32, "matern52": MATERN52, "ratquad": RATQUAD,
               "rq": RATQUAD, "periodic": PERIODIC}
MAX_TERMS, MAX_FACTORS = 4, 2


class Factor:
    """One isotropic factor: kind in {expquad, matern32, matern52, ratquad, periodic}; ``aux`` is RatQuad's alpha or
    Periodic's period.  ``fixed_aux`` keeps it out of the sampled / optimised parameters (the reference pins
    period_length = 1, co2_bayesian_sgpr_hmc.py:79-80)."""

    def __init__(self, kind: str, ls: float, aux: float = 0.0, fixed_aux: bool = False):
        self.kind = _FACTOR_IDS[kind.lower()]
        self.ls, self.aux, self.fixed_aux = float(ls), float(aux), bool(fixed_aux)
        if self.kind in (RATQUAD, PERIODIC) and not self.aux > 0.0:
            raise ValueError("ratquad needs alpha > 0, periodic needs period > 0")


class CompositeKernel:
    """terms: [(amplitude_sd, [Factor, ...]), ...]; k = sum_t amplitude_sd_t**2 * prod_f factor_tf."""

    def __init__(self, terms: Sequence[Tuple[float, Sequence[Factor]]]):
        if not 1 <= len(terms) <= MAX_TERMS:
            raise ValueError("1..%d terms" % MAX_TERMS)
        self.terms = [(float(a), list(f)) for a, f in terms]
        for _, f in self.terms:
            if not 1 <= len(f) <= MAX_FACTORS:
                raise ValueError("1..%d factors per term" % MAX_FACTORS)

    # ------------------------------------------------------------------ parameter block <-> named parameters
    def block(self) -> List[float]:
        b = [0.0] * COMP_LEN
        b[0] = float(len(self.terms))
        for t, (amp, facs) in enumerate(self.terms):
            base = 1 + 8 * t
            b[base], b[base + 1] = amp * amp, float(len(facs))
            for f, fac in enumerate(facs):
                fb = base + 2 + 3 * f
                b[fb], b[fb + 1], b[fb + 2] = float(fac.kind), fac.ls, fac.aux
        return b

    def free_parameters(self) -> List[Tuple[str, int, str]]:
        """(name, block slot, role) of every positive parameter, in a fixed order: role 'amp' (the block stores
        amp**2), 'ls' or 'aux'."""
        out = []
        for t, (_, facs) in enumerate(self.terms):
            base = 1 + 8 * t
            out.append(("amp_%d" % t, base, "amp"))
            for f, fac in enumerate(facs):
                fb = base + 2 + 3 * f
                out.append(("ls_%d_%d" % (t, f), fb + 1, "ls"))
                if fac.kind in (RATQUAD, PERIODIC) and not fac.fixed_aux:
                    out.append(("aux_%d_%d" % (t, f), fb + 2, "aux"))
        return out

    def values(self) -> List[float]:
        """Current values of ``free_parameters()`` (amplitudes as standard deviations)."""
        b = self.block()
        return [math.sqrt(b[s]) if role == "amp" else b[s] for _, s, role in self.free_parameters()]

    def with_values(self, vals: Sequence[float]) -> "CompositeKernel":
        it = iter(float(v) for v in vals)
        terms = []
        for amp, facs in self.terms:
            a = next(it)
            nf = []
            for fac in facs:
                ls = next(it)
                aux = fac.aux
                if fac.kind in (RATQUAD, PERIODIC) and not fac.fixed_aux:
                    aux = next(it)
                nf.append(_clone_factor(fac, ls, aux))
            terms.append((a, nf))
        return CompositeKernel(terms)


def _clone_factor(fac: Factor, ls: float, aux: float) -> Factor:
    f = Factor.__new__(Factor)
    f.kind, f.ls, f.aux, f.fixed_aux = fac.kind, float(ls), float(aux), fac.fixed_aux
    return f


def co2_kernel(n_per=1.0, l_psmooth=1.0, l_pdecay=1.0, n_med=1.0, l_med=1.0, alpha=1.0, n_trend=1.0, l_trend=1.0,
               n_noise=1.0, l_noise=1.0, period=1.0) -> CompositeKernel:
    """The reference's CO2 covariance, PyMC3 side (experiments/co2_bayesian_sgpr_hmc.py:107-149); period fixed."""
    return CompositeKernel([
        (n_per, [Factor("periodic", l_psmooth, period, fixed_aux=True), Factor("expquad", l_pdecay)]),
        (n_med, [Factor("ratquad", l_med, alpha)]),
        (n_trend, [Factor("expquad", l_trend)]),
        (n_noise, [Factor("matern32", l_noise)]),
    ])


# the reference's priors on the log-parameters of the CO2 model (co2_bayesian_sgpr_hmc.py:107-141): Normal(0, sd)
CO2_LOG_PRIOR_SD = {"amp_0": 3.0, "ls_0_0": 1.0, "ls_0_1": 0.1, "amp_1": 3.0, "ls_1_0": 3.0, "aux_1_0": 0.1,
                    "amp_2": 3.0, "ls_2_0": 1.0, "amp_3": 3.0, "ls_3_0": 1.0}


class CompositeHmcTarget:
    """logp(theta) and gradient for theta = [log of every free kernel parameter ..., log sigma].

    Kernel parameters: log p ~ Normal(0, sd_p) (the reference declares ``log_x = pm.Normal`` and uses exp(log_x), so the
    sampled variable is the log itself and there is no Jacobian term); sigma ~ HalfNormal(1), log-transformed as PyMC3
    does for positive variables (Jacobian + log sigma).  A failed Cholesky gives -inf, never an exception.
    """

    def __init__(self, bound: CollapsedBound, Z, kernel: CompositeKernel, log_prior_sd: Optional[dict] = None):
        if bound.kernel != "composite":
            raise ValueError("CompositeHmcTarget needs CollapsedBound(kernel='composite')")
        self.bound, self.kernel = bound, kernel
        self.Z = bound._prep_Z(Z)
        self.params = kernel.free_parameters()
        sd = log_prior_sd or {}
        self.sd = [float(sd.get(name, 3.0)) for name, _, _ in self.params]
        self.ndim = len(self.params) + 1

    def constrain(self, theta):
        """Trace row: 'ls' holds every free kernel parameter (``kernel.free_parameters()`` order, amplitudes as
        standard deviations), 'sig_n' the noise sd; 'sig_f' is kept at 1 so ``Trace`` keeps the reference's columns."""
        th = [float(v) for v in theta]
        vals = [math.exp(v) for v in th[:-1]]
        return {"ls": vals, "sig_f": 1.0, "sig_n": math.exp(th[-1]), "kernel": self.kernel.with_values(vals)}

    def start(self):
        """PyMC3's test point: the prior mean of every Normal log-parameter (0) and sigma = 1."""
        return [0.0] * self.ndim

    _ROLE_ID = {"amp": 0, "ls": 1, "aux": 2}

    def device_description(self):
        """The ``composite=`` argument of ``engine.small_eval`` / ``small_nuts``: the structure (term / factor types, fixed
        periods) and the table (block slot, role, prior sd) of the sampled parameters."""
        return {"structure": self.kernel.block(),
                "free": [(slot, self._ROLE_ID[role], sd) for (_, slot, role), sd in zip(self.params, self.sd)]}

    def device_sampler_ok(self, n_draws_total=None, max_treedepth=10):
        """True when ``hmc.sample_nuts_device`` can run this target (``sgp_small_nuts_composite``: at most 17 sampled parameters;
        see ``targets.device_sampler_ok``)."""
        return self.ndim <= 18 and device_sampler_ok(self.bound, "small_nuts", self.Z.shape[0], False, n_draws_total, max_treedepth)

    def run_on_device(self, q0, tune, n_samples, rng_state, **sampler_opts):
        b = self.bound
        return b.engine.small_nuts(b.X, b.y, self.Z, q0, tune, n_samples, rng_state, jitter=b.jitter, kernel=b.kernel,
                                   composite=self.device_description(), **sampler_opts)

    def logp_and_grad(self, theta):
        th = as_floats(theta)
        bad = (-math.inf, [0.0] * self.ndim)
        if not in_range(th):
            return bad
        b = self.bound
        if single_launch_ok(b, self.Z.shape[0]):
            if not all(abs(v) < 150.0 for v in th):  # (the launch's own exp range)
                return bad
            r = single_launch_eval(b, self.Z, th, self.ndim, composite=self.device_description())
            return bad if r is None else r[:2]
        vals = [math.exp(v) for v in th[:-1]]
        sigma = math.exp(th[-1])
        kern = self.kernel.with_values(vals)
        F, g = self.bound.value_and_grad(self.Z, kern.block(), 1.0, sigma * sigma, raise_on_fail=False)
        if not math.isfinite(F):
            return bad
        gb = g["ls"]
        lp, grad = F, []
        for (name, slot, role), v, t, sd in zip(self.params, vals, th[:-1], self.sd):
            dF = float(gb[slot])
            dF_dlog = 2.0 * v * v * dF if role == "amp" else v * dF  # block stores amp**2
            lp += -0.5 * (t / sd) ** 2 - math.log(sd) - 0.5 * math.log(2.0 * math.pi)
            grad.append(dF_dlog - t / (sd * sd))
        # sigma ~ HalfNormal(1): log density 0.5 log(2/pi) - sigma^2/2, plus the log-transform Jacobian log sigma
        lp += 0.5 * math.log(2.0 / math.pi) - 0.5 * sigma * sigma + th[-1]
        grad.append(2.0 * sigma * sigma * g["s2"] - sigma * sigma + 1.0)
        return lp, grad

    def logp(self, theta):
        return self.logp_and_grad(theta)[0]


# ---------------------------------------------------------------------------------------------------------------------
# SGPMC + HMC with a composite kernel, white noise and a linear mean function (the reference's experiments/co2_sgpmc.py)
# ---------------------------------------------------------------------------------------------------------------------
def co2_sgpmc_kernel() -> CompositeKernel:
    """The covariance of experiments/co2_sgpmc.py:66-73 without its White term (``CompositeSgpmcTarget(white=...)`` carries that):
    Periodic(SquaredExponential, period 1, fixed) * Matern52 with ONE variance (the Matern's is frozen at 1, :73) + RationalQuadratic
    + SquaredExponential(variance log(2)^2) + Matern52, every other value at GPflow's default 1.
    [UPSTREAM] GPflow's ``Periodic(base_kernel=SquaredExponential)`` is taken to be variance * exp(-1/2 sum_j sin^2(pi r_j / period) /
    lengthscale^2) -- its docstring as recalled, equal to SGP_FAC_PERIODIC; GPflow is not installed and nothing was checked against it."""
    return CompositeKernel([
        (1.0, [Factor("periodic", 1.0, 1.0, fixed_aux=True), Factor("matern52", 1.0)]),
        (1.0, [Factor("ratquad", 1.0, 1.0)]),
        (math.log(2.0), [Factor("expquad", 1.0)]),
        (1.0, [Factor("matern52", 1.0)]),
    ])


# experiments/co2_sgpmc.py:61-90,109, under the names of ``CompositeSgpmcTarget.names`` for ``co2_sgpmc_kernel()``
CO2_SGPMC_PRIORS = {
    "variance_0": ("halfnormal", 2.0), "lengthscale_0_0": ("gamma", 4.0, 3.0), "lengthscale_0_1": ("gamma", 10.0, 0.075),
    "variance_1": ("halfnormal", 0.5), "lengthscale_1_0": ("gamma", 2.0, 0.75), "alpha_1_0": ("gamma", 5.0, 2.0),
    "variance_2": ("halfnormal", 2.0), "lengthscale_2_0": ("gamma", 4.0, 0.1),
    "variance_3": ("halfnormal", 0.5), "lengthscale_3_0": ("gamma", 2.0, 4.0),
    "white": ("halfnormal", 0.25), "mean_A": ("normal", 0.0, 3.0), "mean_b": ("normal", 0.0, 3.0), "noise_variance": ("gamma", 2.0, 1.0),
}


def _log_prior(spec, c):
    """(log density, its derivative) of one prior at the value c: ("gamma", concentration, rate) | ("halfnormal", scale) |
    ("normal", mean, sd)."""
    kind = spec[0]
    if kind == "gamma":
        a, b = float(spec[1]), float(spec[2])
        return a * math.log(b) - math.lgamma(a) + (a - 1.0) * math.log(c) - b * c, (a - 1.0) / c - b
    if kind == "halfnormal":
        s = float(spec[1])
        return 0.5 * math.log(2.0 / math.pi) - math.log(s) - 0.5 * (c / s) ** 2, -c / (s * s)
    if kind == "normal":
        m, s = float(spec[1]), float(spec[2])
        return -0.5 * math.log(2.0 * math.pi) - math.log(s) - 0.5 * ((c - m) / s) ** 2, -(c - m) / (s * s)
    raise ValueError("unknown prior %r: 'gamma', 'halfnormal' or 'normal'" % (kind,))


class CompositeSgpmcTarget(SgpmcTargetBase):
    """logp(q) and its gradient for HMC over the hyper-parameters and the whitened inducing values of GPflow's ``SGPMC`` with a
    sum-of-products kernel, an optional White term and an optional linear mean function -- the model of experiments/co2_sgpmc.py.

    q, unconstrained, in this order (``names``): per term of ``kernel`` ``variance_t`` (the block's amp2 slot: GPflow's parameter, not
    the amplitude sd), per factor ``lengthscale_t_f`` and each free ``alpha_t_f`` (ratquad) / ``period_t_f`` (an unfixed period);
    ``white`` (when ``white`` is not None: its start value); ``noise_variance`` (Gaussian likelihood only, floor 1e-6); ``mean_A`` (d)
    and ``mean_b`` (``mean="linear"``: m(x) = x.A + b); ``V`` (M).  Positive entries go through softplus with log sigmoid(x) added for
    the transform, as ``SgpmcTarget`` does; the mean coefficients are unconstrained.  ``priors``: name -> ("gamma", concentration,
    rate) | ("halfnormal", scale) | ("normal", mean, sd) on the constrained value; a name without an entry contributes nothing
    ([UPSTREAM] GPflow's ``log_prior_density`` as recalled).  V ~ N(0, I).

    The density F(v, theta) and its adjoints are stated in include/sgp.h (sgp_sgpmc_comp_rows).  One evaluation is
    ``kuu(jitter + white)`` -> ``kuu_factor`` -> ``sgpmc_comp_rows`` -> ``sgpmc_lik_tail`` -> ``sgpmc_comp_bwd`` -> ``kuu_bwd``, with one
    result buffer and one device-to-host copy (tr(Kuubar) for dF/dwhite and the two sums of the mean function ride in it); transforms,
    priors and the chain rule run on the host.  A non-zero ``kuu_factor`` status or a non-finite value gives (-inf, zeros); a device
    time-out raises ``SgpTimeoutError``.  Z is fixed per evaluation (``set_Z`` replaces it); there is no dF/dZ.  One process."""

    _NAME = "CompositeSgpmcTarget"

    def __init__(self, X, y, Z, kernel: CompositeKernel, priors=None, white=None, mean=None, likelihood="gaussian", jitter=1e-4,
                 engine=None):
        if mean not in (None, "linear"):
            raise ValueError("mean is None or 'linear' (got %r)" % (mean,))
        if white is not None and not float(white) > 0.0:
            raise ValueError("white is None (no White term) or its positive start value")
        self._intake(X, y, likelihood, engine)
        self.kernel, self.jitter, self.mean = kernel, float(jitter), mean
        self.priors = dict(priors or {})
        self._structure = kernel.block()
        # the theta entries: (name, role, block slot or coefficient index, start value); roles amp / ls / aux / white / noise are positive
        ent = []
        for (pname, slot, role), val in zip(kernel.free_parameters(), kernel.values()):
            t_f = pname.split("_", 1)[1]
            if role == "amp":
                ent.append(("variance_" + t_f, role, slot, val * val))
            elif role == "ls":
                ent.append(("lengthscale_" + t_f, role, slot, val))
            else:
                ent.append((("alpha_" if int(self._structure[slot - 2]) == RATQUAD else "period_") + t_f, role, slot, val))
        if white is not None:
            ent.append(("white", "white", -1, float(white)))
        if likelihood == "gaussian":
            ent.append(("noise_variance", "noise", -1, 1.0))
        if mean == "linear":
            ent += [("mean_A", "A", j, 1.0) for j in range(self.d)] + [("mean_b", "b", 0, 0.0)]
        self._entries = ent
        self.n_theta = len(ent)
        for name in self.priors:
            if name not in {e[0] for e in ent}:
                raise ValueError("a prior is given for %r, which this target does not sample (%s)" % (name, ", ".join(self.names)))
            _log_prior(self.priors[name], 1.0)
        self.set_Z(Z)

    @property
    def names(self):
        """The theta entries in the order of q (``mean_A`` once per input dimension), without ``V``."""
        return [e[0] for e in self._entries]

    def start(self):
        """[UPSTREAM] GPflow's defaults as recalled: variances, lengthscales, alpha, white and the likelihood variance 1, A = 1, b = 0,
        V = 0 -- with ``kernel``'s own values (``co2_sgpmc_kernel()``: variance log(2)^2 on the trend) and ``white``'s start value."""
        out = []
        for _, role, _, val in self._entries:
            out.append(val if role in ("A", "b") else _softplus_inv(val - (_SGPMC_NOISE_FLOOR if role == "noise" else 0.0)))
        return out + [0.0] * self.M

    def unpack(self, q):
        """(block, white, noise variance or None, A list or None, b, constrained theta list) of a position."""
        x = as_floats(q)
        block, white, s2, A, b, cons = list(self._structure), 0.0, None, None, 0.0, []
        for (_, role, idx, _), t in zip(self._entries, x):
            if role in ("A", "b"):
                c = t
            else:
                c = _softplus(t) + (_SGPMC_NOISE_FLOOR if role == "noise" else 0.0)
            cons.append(c)
            if role in ("amp", "ls", "aux"):
                block[idx] = c
            elif role == "white":
                white = c
            elif role == "noise":
                s2 = c
            elif role == "A":
                A = (A or []) + [c]
            else:
                b = c
        return block, white, s2, A, b, cons

    def constrain(self, q):
        """The constrained values of a position under ``names`` (``mean_A`` as an array), ``V``, and ``kernel`` (a ``CompositeKernel``)."""
        x = as_floats(q)
        block, _, _, A, _, cons = self.unpack(x)
        c = {name: v for (name, role, _, _), v in zip(self._entries, cons) if role != "A"}
        if A is not None:
            c["mean_A"] = np.asarray(A, dtype=np.float64)
        c["V"] = np.asarray(x[self.n_theta:], dtype=np.float64)
        c["kernel"] = self.kernel.with_values([math.sqrt(block[s]) if r == "amp" else block[s] for _, s, r in self.kernel.free_parameters()])
        return c

    def _eval(self, q, want_grad):
        x = as_floats(q)
        d, M, N, e, nt = self.d, self.M, self.N, self.engine, self.n_theta
        if len(x) != self.ndim:
            raise ValueError("the position has %d entries, expected %d theta + M = %d" % (len(x), nt, self.ndim))
        bad = (-math.inf, [0.0] * self.ndim if want_grad else None)
        positive = [role not in ("A", "b") for _, role, _, _ in self._entries]
        if not all(math.isfinite(t) for t in x) or not all(abs(t) < 700.0 for t, p in zip(x, positive) if p):
            return bad
        block, white, s2, A, b, cons = self.unpack(x)
        if not all(c > 0.0 for c, p in zip(cons, positive) if p):   # softplus underflowed: outside the representable range
            return bad
        self.n_evals += 1
        linear = A is not None
        # extras of the result buffer: [dF/d block (COMP_LEN) + kuu_bwd's amplitude slot | vbar (M) | tr Kuubar | sum dmu x (d) | sum dmu].
        # The amplitude slot exists because kuu_bwd's layout has it; the composite path never writes it and nothing here reads it: it
        # holds whatever torch.empty left (clearing it would cost a launch per evaluation).
        extra = COMP_LEN + 1 + M + 1 + d + 1 if want_grad else 0
        result = e.result_buffer(extra)
        buf = result[0]
        head = buf.numel() - extra
        Kuu = e.kuu(self.Z, block, 1.0, self.jitter + white, "composite")   # White is K_uu's diagonal and k(x, x) only
        linv, _ = e.kuu_factor(Kuu, info=result[2])                         # the evaluation's status word is the K_uu status
        up = torch.tensor(x[nt:] + (A + [b] if linear else []), dtype=torch.float64).to(e.device)
        v = up[:M]
        mean = torch.addmv(up[M + d:].expand(N), self.X, up[M:M + d]) if linear else None
        t_keep = self._t_for()
        rows = e.sgpmc_comp_rows(self.X, self.y, self.Z, block, white, s2 if s2 is not None else 1.0, v, linv, t_keep, self.likelihood,
                                 mean=mean, want_adjoints=want_grad)
        o_g, o_v, o_t = head, head + COMP_LEN + 1, head + COMP_LEN + 1 + M
        res = e.sgpmc_lik_tail(rows, v, N, linv, with_adjoints=want_grad, result=result, **({"vbar_out": buf[o_v:o_t]} if want_grad else {}))
        if want_grad:
            g = buf[o_g:o_v]
            e.sgpmc_comp_bwd(self.X, rows["dmu"], self.Z, block, t_keep, linv, res["bbar"], out=g)
            e.kuu_bwd(self.Z, block, 1.0, res["Kuubar"], g, "composite")
            torch.sum(torch.diagonal(res["Kuubar"]), dim=0, keepdim=True, out=buf[o_t:o_t + 1])
            if linear:
                torch.mv(self.X.t(), rows["dmu"], out=buf[o_t + 1:o_t + 1 + d])
                torch.sum(rows["dmu"], dim=0, keepdim=True, out=buf[o_t + 1 + d:o_t + 2 + d])
        host = buf.detach().to("cpu")   # the one host round trip
        o, info = e.read_result(host)
        if info < 0:
            raise SgpTimeoutError()
        F = float(o[0])
        if info != 0 or not math.isfinite(F):
            return bad
        logp = F
        pri = []
        for (name, _, _, _), c, t, p in zip(self._entries, cons, x, positive):
            lp, dlp = _log_prior(self.priors[name], c) if name in self.priors else (0.0, 0.0)
            sg = _sigmoid(t) if p else 1.0
            if not sg > 0.0:
                return bad
            logp += lp + (math.log(sg) if p else 0.0)
            pri.append((dlp, sg))
        if not want_grad:
            return logp, None
        hl = host.tolist()
        gb, sdv, tr = hl[o_g:o_g + COMP_LEN], float(o[4]) * N, hl[o_t]
        grad = []
        for (_, role, idx, _), (dlp, sg), p in zip(self._entries, pri, positive):
            if role == "amp":       # k(x_n, x_n) holds every amp2 slot: + sum_n dv_n (N out[4], as SgpmcTarget adds it)
                dF = gb[idx] + sdv
            elif role in ("ls", "aux"):
                dF = gb[idx]
            elif role == "white":
                dF = tr + sdv
            elif role == "noise":
                dF = float(o[3])
            else:
                dF = hl[o_t + 1 + idx] if role == "A" else hl[o_t + 1 + d]
            grad.append((dF + dlp) * sg + (1.0 - sg) if p else dF + dlp)
        grad += hl[o_v:o_t]
        if not all(math.isfinite(t) for t in grad):
            return bad
        return logp, grad

    def logp(self, q):
        return self._eval(q, False)[0]

    def logp_and_grad(self, q):
        return self._eval(q, True)


# ---------------------------------------------------------------------------------------------------------------------
# The reference's CO2 model class (experiments/co2_bayesian_sgpr_hmc.py:58-300): its own copy of BayesianSparseGPR_HMC with
# the composite covariance -- warm start with Adam on every raw parameter, then Adam on Z alone against the bound averaged
# over the current NUTS trace, with NUTS phases at the scheduled iterations.
# ---------------------------------------------------------------------------------------------------------------------
def _inv_softplus(v: float) -> float:
    return v + math.log(-math.expm1(-v)) if v < 30.0 else v


class _CompositeBoundFn(torch.autograd.Function):
    """F(values, s2, Z) / N for a composite kernel; ``values`` = the free parameters in ``CompositeKernel.free_parameters()``
    order (amplitudes as standard deviations).  Gradients from the HIP library (dF/d block -> chain rule to the values)."""

    @staticmethod
    def forward(ctx, values, s2, Z, model):
        cb = model.bound
        kern = model.kernel.with_values([float(v) for v in values.detach().tolist()])
        need = any(ctx.needs_input_grad[:3])
        if need:
            Fv, g = cb.value_and_grad(Z.detach(), kern.block(), 1.0, float(s2), want_gz=bool(ctx.needs_input_grad[2]))
            gv = []
            for (_, slot, role), v in zip(model.params, values.detach().tolist()):
                dF = float(g["ls"][slot])
                gv.append(2.0 * v * dF if role == "amp" else dF)  # the block stores amp**2
            ctx.g = (torch.tensor(gv, dtype=torch.float64), float(g["s2"]), g["Z"])
        else:
            Fv, _ = cb.value(Z.detach(), kern.block(), 1.0, float(s2))
            ctx.g = None
        ctx.N = cb.N
        ctx.meta = (values.shape, values.device, Z.shape)
        return torch.tensor(Fv / cb.N, dtype=torch.float64, device=values.device)

    @staticmethod
    def backward(ctx, gout):
        gv, gs2, gz = ctx.g
        vshape, vdev, zshape = ctx.meta
        s = gout / ctx.N
        out_v = (gv.to(vdev).reshape(vshape) * s) if ctx.needs_input_grad[0] else None
        out_s = (torch.as_tensor(gs2, dtype=torch.float64, device=vdev) * s).reshape(()) if ctx.needs_input_grad[1] else None
        out_z = (gz.reshape(zshape) * s.to(gz.device)) if ctx.needs_input_grad[2] else None
        return out_v, out_s, out_z, None


class CompositeBayesianSparseGPR_HMC(torch.nn.Module):  # noqa: N801  (after the reference's class name)
    """Collapsed sparse GP regression with a sum-of-products covariance, hyper-parameters sampled by NUTS at scheduled
    iterations -- the class of experiments/co2_bayesian_sgpr_hmc.py:58-300 on the HIP core.

    Parameters (all learnable in the warm start): ``raw_values`` (softplus -> the kernel's free parameters, amplitudes as
    standard deviations), ``raw_noise`` (softplus -> noise variance, + 1e-4 as GPyTorch's GaussianLikelihood) and
    ``inducing_points``.  ``train_model`` returns (losses, trace_hyper, trace_step_size, trace_perf_time) like the reference
    (:186-253); ``train_fixed_model`` is its HMC-only run (:257-277, 500 tune / 100 draws)."""

    def __init__(self, train_x, train_y, kernel: CompositeKernel, Z_init, log_prior_sd: Optional[dict] = None, engine=None,
                 jitter: float = 1e-6, noise: float = 0.1, seed: Optional[int] = None):
        super().__init__()
        if train_x.dim() == 1:
            train_x = train_x[:, None]
        self.bound = CollapsedBound(train_x, train_y, kernel="composite", jitter=jitter, engine=engine)
        self.kernel = kernel
        self.params = kernel.free_parameters()
        self.log_prior_sd = dict(log_prior_sd or {})
        dev = self.bound.engine.device
        self.raw_values = torch.nn.Parameter(torch.tensor([_inv_softplus(v) for v in kernel.values()], dtype=torch.float64))
        self.raw_noise = torch.nn.Parameter(torch.tensor(_inv_softplus(max(noise - 1e-4, 1e-6)), dtype=torch.float64))
        Z = torch.as_tensor(Z_init, dtype=torch.float64)
        self.inducing_points = torch.nn.Parameter((Z[:, None] if Z.dim() == 1 else Z).clone().to(dev))
        self._seed, self._n_hmc_calls = seed, 0
        self.device_sampler = True

    # ------------------------------------------------------------------ parameters
    def values(self) -> torch.Tensor:
        return torch.nn.functional.softplus(self.raw_values)

    def noise(self) -> torch.Tensor:
        return torch.nn.functional.softplus(self.raw_noise) + 1e-4

    def current_kernel(self) -> CompositeKernel:
        return self.kernel.with_values([float(v) for v in self.values().detach().tolist()])

    def freeze_kernel_hyperparameters(self):
        self.raw_values.requires_grad = False
        self.raw_noise.requires_grad = False

    def update_model_to_hyper(self, hyper_sample):
        """Set kernel parameters and noise to one draw of the trace (reference :162-184); period lengths stay fixed."""
        with torch.no_grad():
            vals = np.asarray(hyper_sample["ls"], dtype=np.float64)
            self.raw_values.copy_(torch.tensor([_inv_softplus(float(v)) for v in vals], dtype=torch.float64))
            self.raw_noise.copy_(torch.tensor(_inv_softplus(max(float(hyper_sample["sig_n"]) ** 2 - 1e-4, 1e-12)), dtype=torch.float64))

    # ------------------------------------------------------------------ bound
    def neg_bound_per_datum(self):
        return -_CompositeBoundFn.apply(self.values(), self.noise(), self.inducing_points, self)

    def sample_optimal_variational_hyper_dist(self, n_samples, Z_opt, tune, sampler_params=None):
        """NUTS over the log-parameters with Z fixed (reference :99-160).  Starts at the current parameter values."""
        Z = torch.as_tensor(np.asarray(Z_opt), dtype=torch.float64)
        target = CompositeHmcTarget(self.bound, Z, self.current_kernel(), self.log_prior_sd)
        start = [math.log(float(v)) for v in self.values().detach().tolist()] + [0.5 * math.log(float(self.noise().detach()))]
        scale = 0.25 if not sampler_params else sampler_params.get("step_scale", 0.25)
        fn = sample_nuts_device if (self.device_sampler and target.device_sampler_ok(n_samples + tune)) else sample_nuts
        return fn(target, n_samples, tune, seed=next_seed(self), start=start, step_scale=scale)

    def train_model(self, optimizer, max_steps=10000, hmc_scheduler=(200, 500, 1000, 1500), verbose=False,
                    num_tune_long=200, num_samples_long=50, num_tune_short=25, num_samples_short=10):
        return few_host_threads(self._train_model)(optimizer, max_steps, list(hmc_scheduler), verbose, num_tune_long,
                                                    num_samples_long, num_tune_short, num_samples_short)

    def _train_model(self, optimizer, max_steps, hmc_scheduler, verbose, num_tune_long, num_samples_long, num_tune_short,
                     num_samples_short):
        self.train()
        losses, trace_hyper, trace_step_size, trace_perf_time = [], None, [], []
        for n_iter in range(max_steps):
            optimizer.zero_grad()
            if n_iter < hmc_scheduler[0]:  # warm start: every raw parameter
                loss = self.neg_bound_per_datum()
                losses.append(loss.item())
                loss.backward()
                optimizer.step()
                continue
            self.freeze_kernel_hyperparameters()
            if trace_hyper is not None:  # the bound averaged over the current trace, differentiable in Z only
                loss = 0.0
                for i in range(len(trace_hyper)):
                    self.update_model_to_hyper(trace_hyper[i])
                    loss = loss + self.neg_bound_per_datum() / len(trace_hyper)
                if verbose:
                    print('Iter %d/%d - Loss: %.3f ' % (n_iter, max_steps, loss.item()))
                losses.append(loss.item())
                loss.backward()
                optimizer.step()
            if n_iter in hmc_scheduler:
                Z_opt = self.inducing_points.detach().cpu().numpy()
                long_phase = n_iter in (hmc_scheduler[0], hmc_scheduler[-1])
                trace_hyper = self.sample_optimal_variational_hyper_dist(num_samples_long if long_phase else num_samples_short, Z_opt,
                                                                         num_tune_long if long_phase else num_tune_short)
                trace_step_size.append(trace_hyper.get_sampler_stats('step_size')[0])
                trace_perf_time.append(trace_hyper.get_sampler_stats('perf_counter_diff').sum())
        return losses, trace_hyper, trace_step_size, trace_perf_time

    def train_fixed_model(self, num_tune=500, num_samples=100):
        """NUTS over the hyper-parameters with Z fixed at its current value (reference :257-277)."""
        trace = self.sample_optimal_variational_hyper_dist(num_samples, self.inducing_points.detach().cpu().numpy(), num_tune)
        return trace_summary(trace)

    # ------------------------------------------------------------------ predictive
    def posterior_predictive(self, test_x, full_cov=False):
        """(mean, variance[, covariance]) of y* at test_x, observation noise included (reference :283-300)."""
        with torch.no_grad():
            mean, var, cov = self.bound.predict(test_x, self.inducing_points.detach(), self.current_kernel().block(), 1.0,
                                                float(self.noise()), pred_noise=True, full_cov=full_cov)
        return (mean, var, cov) if full_cov else (mean, var)

    def mixture_posterior_predictive(self, test_x, trace_hyper):
        """One (mean, variance) per draw of the trace (reference :302-340); the model is left at the last draw."""
        out = []
        for i in range(len(trace_hyper)):
            self.update_model_to_hyper(trace_hyper[i])
            out.append(self.posterior_predictive(test_x))
        return out
