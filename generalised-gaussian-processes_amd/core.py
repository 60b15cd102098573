"""CollapsedBound: the hot path as one object -- F(theta, Z), its gradient and the predictive.

Reference call sites this replaces (paths relative to the reference repo):
  * ``-mll(model(train_x), train_y)`` on ``SparseGPR``            models/sgpr.py:123-125
  * ``pm.gp.MarginalSparse(approx="VFE").marginal_likelihood``   models/bayesian_sgpr_hmc.py:66,71
  * ``likelihood(model(test_x))``                                 models/sgpr.py:150-160

Data layout: X (N_local x d) and y (N_local) are resident on this rank's GPU for the whole run
(row-sharded contiguously across ranks, never moved); Z (M x d) and the hyper-parameters are
replicated.  One evaluation =
    pass 1 on the local rows  ->  ONE all-reduce of the packed [Phi | b | yy | kappa] buffer
    (RCCL over xGMI when world_size > 1)  ->  O(M^3) tail replicated on every rank (deterministic,
    so no broadcast)  [-> pass 2 on the local rows -> one small all-reduce of the gradients].
"""
from __future__ import annotations

import math

import torch

try:  # torch.distributed is plumbing; single-process use never touches it
    import torch.distributed as dist
except Exception:  # pragma: no cover
    dist = None

from ._lib import COMP_LEN, OUT_F, OUT_LOGMARG, OUT_S2BAR, OUT_TRACE


class NotPositiveDefiniteError(RuntimeError):
    """Raised (Adam path) when a Cholesky pivot is non-positive; ``info`` is the LAPACK-style index."""

    def __init__(self, info):
        super().__init__("matrix not positive definite: leading minor of order %d (1..M: Kuu, M+1..2M: B)" % info)
        self.info = info


class SgpTimeoutError(RuntimeError):
    """The single-launch Cholesky gave up waiting for a tile (status word SGP_INFO_TIMEOUT): a device scheduling
    problem, not a property of the matrix.  Always raised -- never turned into logp = -inf, which would bias a chain."""

    def __init__(self):
        super().__init__("device time-out inside the dataflow Cholesky (SGP_INFO_TIMEOUT): outputs are invalid")
        self.info = SGP_INFO_TIMEOUT


SGP_INFO_TIMEOUT = -7777


def few_host_threads(fn):
    """Decorator for the host-driven loops (training, sampling): the host side of a step is a handful of torch operations
    on tensors with d + 2 ... M entries (raw-parameter transforms, a 4 x 4 Cholesky of q(log theta), optimizer updates).
    With torch's default intra-op pool -- one thread per host core, 128-256 on the GPU boxes -- every such operation pays the
    pool's wake-up, and the spinning workers starve the HIP runtime's own threads: a BayesianSVGP minibatch step took 37.6 ms
    with 128 threads and 4.4 ms with one (`tools/bsvgp_rates.py`).  The cap (4) is lifted again when the loop returns."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        n = torch.get_num_threads()
        if n <= 4:
            return fn(*args, **kwargs)
        torch.set_num_threads(4)
        try:
            return fn(*args, **kwargs)
        finally:
            torch.set_num_threads(n)

    return wrapped


# ---------------------------------------------------------------------------------------------
# The streaming-order guard, host side.  Three evaluation orders ("tiers") compute the same bound:
#   0 streaming  Phi = K_uf K_fu streamed, W = L^-1 Phi L^-T in the tail           (the N >> M design; fastest)
#   1 extended   the same from an exact Phi and a double-double sandwich            (values hold 2^14 x further; its explicit-Phibar
#                                                                                    gradients 3 x further)
#   2 whitened   PyMC3's op order, A = L^-1 K_uf first                               (always accurate; two more N M^2 products)
# Every evaluation reports the library's first-order estimate of the streaming order's error at ITS theta (exact in tiers 0 and 1,
# which form Phi; tier 2 can only report the upper bound).  `required_tier` -- a pure function -- says which tier that estimate asks
# for; an evaluation that ran in a lower tier is repeated in the required one.  What is remembered between evaluations (GuardState)
# only decides where the next one STARTS, so that a sampler sitting in a guarded region does not pay a wasted streaming attempt per
# leapfrog; it never decides what is accepted.  Consequence, documented in include/sgp.h / INTEGRATION.md: the bits of F(theta) depend
# on the tier (tiers agree to ~1e-9 per datum), and the tier an evaluation is ACCEPTED in can be higher than required when the
# previous evaluations suggested it (never lower).  All inputs of these decisions are replicated numbers: ranks decide alike.
# ---------------------------------------------------------------------------------------------
TIER_STREAMING, TIER_EXTENDED, TIER_WHITENED = 0, 1, 2


def required_tier(estimate, tol, reach, extended_ok):
    """The cheapest tier that meets `tol` at a theta whose streaming-order error estimate is `estimate`.  `reach`: how many times the
    tolerance the extended order covers for this kind of evaluation (values / gradients); `extended_ok`: that order exists here."""
    if estimate <= tol:
        return TIER_STREAMING
    if extended_ok and estimate <= reach * tol:  # (NaN / inf fail both comparisons: the whitened order)
        return TIER_EXTENDED
    return TIER_WHITENED


class GuardState:
    """All the guard remembers between evaluations."""

    __slots__ = ("open", "predicted", "ratio")

    def __init__(self):
        self.open = False        # an episode is open: evaluations start in the tier the prediction asks for, without a streaming attempt
        self.predicted = 0.0     # the streaming-order estimate expected at the next theta
        self.ratio = 1.0         # estimate / upper bound at the last evaluation that knew both (predicts the estimate from a whitened one)

    def start_tier(self, tol, reach, extended_ok):
        """Where the next evaluation starts.  Inside an episode never in the streaming order (hysteresis: the episode ends once the
        prediction is below half the tolerance), so a theta hovering around the tolerance does not pay a repeat every other time."""
        if not self.open:
            return TIER_STREAMING
        return TIER_EXTENDED if (extended_ok and self.predicted <= reach * tol) else TIER_WHITENED

    def note_exact(self, estimate, bound, tol):
        """After an evaluation that formed Phi (tiers 0, 1): `estimate` is exact at its theta."""
        if math.isfinite(estimate) and math.isfinite(bound) and bound > 0.0:
            self.ratio = min(1.0, max(estimate / bound, 0.0))
        self.predicted = estimate
        self.open = not (estimate < 0.5 * tol) if self.open else not (estimate <= tol)

    def note_bound(self, bound, tol):
        """After a whitened-order evaluation: only the upper bound is known; the last ratio turns it into a prediction."""
        if math.isfinite(bound) and bound > 0.0:
            self.predicted = self.ratio * bound
            self.open = not (self.predicted < 0.5 * tol)


class Attempt:
    """What ONE attempt of an evaluation produced: the tier, the result buffer (`buf`, with `out` and the status word `info` inside it), what
    pass 1 and the tail left on the device (adjoints: None for a value-only attempt) and, once `_fetch` has run, the host's view -- `host`
    (the copy), `o` (out as floats), `status` (the status word), the packed gradient behind `head`.  `factored`: the route of pass 2 -- L^-T Cw L^-1
    applied factor by factor (whitened order), else the explicit Phibar with or without its trailing word `Phibar_lo` (the extended order forms
    its Phibar FROM a core and still takes this route).  `complete`: everything the caller needs is on the host, so the walk can come back to
    the attempt; `need`: the tier its own estimate names, once `_verdict` has read it."""

    __slots__ = ("tier", "buf", "out", "info", "packed", "Kuu", "linv", "Phibar", "bbar", "Kuubar", "Cw", "Phibar_lo", "factored", "kfu", "kfu_f16",
                 "t_keep", "factors", "reported", "host", "o", "status", "head", "complete", "need")

    def __init__(self, tier, res, head, packed, Kuu, linv, kfu=None, kfu_f16=None, t_keep=None, factored=False):
        get = res.get   # (what engine.bound returned: the adjoints and factors it was asked for)
        self.tier, self.buf, self.out, self.info, self.head = tier, res["buf"], res["out"], res["info"], head
        self.packed, self.Kuu, self.linv, self.kfu, self.kfu_f16, self.t_keep = packed, Kuu, linv, kfu, kfu_f16, t_keep
        self.Phibar, self.bbar, self.Kuubar, self.Cw, self.factors = get("Phibar"), get("bbar"), get("Kuubar"), get("Cw"), get("factors")
        self.Phibar_lo = self.host = self.o = self.status = self.need = None
        self.factored, self.reported, self.complete = factored, False, False


class Plan:
    """What one evaluation settles before its first attempt: see `CollapsedBound._plan`."""

    __slots__ = ("M", "with_grad", "want_gz", "want_factors", "strict", "want_lo", "guard", "reach", "ext_ok", "tier", "nh", "lo_slots",
                 "extra", "early", "lo_check")


WHITENED_ROWS_MIN_WORK = 1 << 26


def whitened_rows_layout(engine, kernel, n_rows, M, min_work=WHITENED_ROWS_MIN_WORK):
    """The whitened pass 1 of a shard of ``n_rows`` rows runs in the streaming layout (``engine.suffstats_whitened_rows``: stationary
    kernels, from ``min_work`` local rows x inducing points) instead of through the chunked routine -- the one rule ``CollapsedBound``
    and ``targets.SgpmcTarget`` share."""
    return hasattr(engine, "suffstats_whitened_rows") and kernel != "composite" and int(n_rows) * int(M) >= min_work


def _world(group):
    if dist is None or not dist.is_available() or not dist.is_initialized():
        return 1
    return dist.get_world_size(group)


class CollapsedBound:
    """Collapsed (Titsias/VFE) sparse-GP bound over a resident row shard.

    Parameters
    ----------
    X, y : local shard, float64, on the engine's device.
    engine : object with the ``HipEngine`` interface; defaults to ``HipEngine()`` (the only product engine).
    jitter : added to diag(Kuu): 0.0 = GPyTorch parity, 1e-6 = PyMC3 ``stabilize`` parity.
    group : torch.distributed process group (None = default group when initialised).
    form : "streaming" -- Phi = K_uf K_fu streamed over the rows, W = L^-1 Phi L^-T in the tail (the N >> M design);
           "whitened"  -- PyMC3's op order, A = L^-1 K_uf materialised, W = A A^T: B = I + W/s2 is positive definite by
                          construction and F keeps 1e-10 accuracy at cond(Kuu) ~ 1e8, for twice the N M^2 work;
           "auto"      -- whitened up to ``WHITENED_MAX_WORK`` row x inducing pairs per rank (the reference's own
                          workloads: N ~ 250-1300, M ~ 100-480), streaming above.
    """

    WHITENED_MAX_WORK = 1 << 20  # local rows x inducing points up to which form="auto" means "whitened"

    def __init__(self, X, y, kernel="rbf", jitter=0.0, engine=None, group=None, form="auto"):
        if engine is None:
            from .engine import HipEngine
            engine = HipEngine(X.device if X.is_cuda else None)
        self.engine = engine
        if X.dim() == 1:
            X = X[:, None]
        self.X = X.to(dtype=torch.float64, device=engine.device).contiguous()
        self.y = y.to(dtype=torch.float64, device=engine.device).reshape(-1).contiguous()
        if self.X.shape[0] != self.y.shape[0]:
            raise ValueError("X has %d rows, y has %d" % (self.X.shape[0], self.y.shape[0]))
        self.d = int(self.X.shape[1])
        self.kernel = kernel
        self.jitter = float(jitter)
        if form not in ("auto", "streaming", "whitened", "extended"):
            raise ValueError("form must be 'auto', 'streaming', 'extended' or 'whitened'")
        self.form = form
        self.group = group
        self.world = _world(group)
        n_local = int(self.X.shape[0])
        if self.world > 1:
            t = torch.tensor([n_local], dtype=torch.int64, device=engine.device)
            dist.all_reduce(t, group=group)
            self.N = int(t.item())
            # form="auto" must come out the same on every rank (the two orders all-reduce different matrices into the
            # same buffer): decide from the LARGEST shard, not from the local one
            dist.all_reduce(t.fill_(n_local), op=dist.ReduceOp.MAX, group=group)
            self._rows_for_form = int(t.item())
        else:
            self.N = n_local
            self._rows_for_form = n_local
        self.n_evals = 0
        self.n_grads = 0
        self.n_collectives = 0
        # K'_fu of the local shard stays resident between pass 1 and pass 2 of one evaluation when it
        # fits the budget (default 64 GiB of the 288 GB HBM); otherwise the library streams it in
        # 16 GiB super-chunks and pass 2 re-assembles.
        self._kfu = None
        self._kfu_f16 = None
        self.kfu_budget_bytes = 64 << 30
        # local rows x inducing points from which the whitened order runs in the streaming layout (engine.suffstats_whitened_rows)
        self.whitened_rows_min_work = WHITENED_ROWS_MIN_WORK
        self.factored_adjoint = True  # whitened order: pass 2 from L^-T Cw L^-1 applied factor by factor (sgp_suffstats_bwd_factored)
        self.fused = True          # single-launch path for small problems (M <= 128, one rank): sgp_small_eval
        self._small = None         # (pinned host theta, device theta, result buffer) of the single-launch path
        self.overlap_tail = True   # factor Kuu on a second HIP stream while pass 1 runs
        self.overlap_min_work = 1 << 21  # local rows x inducing points below which everything stays on one stream
        self.early_check_min_work = 1 << 28  # ... from which value_and_grad reads the status before enqueueing pass 2
        self._side = None          # (side stream, (z_ready, ready) events, {M: (Kuu, L^-1) buffers}) of the two-stream path
        # Guard of the streaming order (form="auto" only; see the block comment above required_tier): the tolerance is per datum on
        # |dF| / N.  extended_level 2 = 39 digit pairs, what the sandwich amplifies is 2^16 smaller (reach 2^14: a factor 4 kept as margin;
        # measured at C5 over 27 theta: <= 1.6e-10 per datum against the whitened order up to estimates of 3e-5,
        # profiles/r04_extended_order_c5.jsonl); level 1 = 34 pairs, 2^8 (0.9 ms cheaper; reach 2^7 then).
        # GRADIENTS: pass 2 of the extended order takes the explicit Phibar, whose product with K_uf cancels -- against the factored pass 2
        # of the whitened order its lengthscale gradients are off by 7e-7 at an estimate of 4e-9, 3e-5 at 8e-8, 3e-2 at 2e-7 (same file):
        # a value + gradient evaluation that must hold 1e-6 takes the extended order within `extended_grad_range` x the tolerance only.
        # A sampler may ask for more (HmcTarget(gradient="sampler"): the value's reach for the gradient as well, see there).
        self.streaming_tol = 1e-9
        self.extended_level = 2
        self.extended_range = 16384.0
        self.extended_grad_range = 3.0
        self.extended_dd_phibar = True   # the extended order's explicit Phibar formed in double-double (sgp_phibar_dd) ...
        self.extended_lo = True            # ... with its trailing word applied in pass 2 where that exists (RBF, K'_fu kept)
        # ... and its reach with the trailing word applied in pass 2 (sgp_suffstats_bwd_lo).  Calibrated at C5 over 34 theta against the factored
        # pass 2 of the whitened order (profiles/r06_extended_order_gradients_dd_phibar.jsonl, ..._ard_...): with both words every cell
        # whose estimate is <= 1e-6 AND whose correction is <= 1e-4 of the gradient is within 6e-7 (the trained ARD thetas of C5: 3e-9 and
        # 2.6e-8 where the leading word alone is off by 1.3e-6 / 4.5e-5 and the fp64-formed matrix by 4.6e-6 / 4.4e-4); isotropic l = 5 is
        # the counter-example that makes the second condition necessary (estimate 1.8e-7, correction 5.5e-4, 8e-6 left).
        self.extended_grad_range_lo = 1000.0
        self.extended_lo_max_correction = 1e-4
        self._lo_skip, self._lo_pause = 0, 0     # gradient evaluations still to start in the whitened order behind a rejection / the current pause (memory only)
        self.last_lo_correction = None
        self.n_lo_rejections = 0
        self.guard = GuardState()
        self.last_estimate = None   # the estimate (exact, or the bound of a whitened evaluation) of the last guarded evaluation
        self.last_tier = None       # the tier the last evaluation was accepted in
        self.n_guard_reruns = 0     # evaluations repeated in a higher tier
        self.n_direct_whitened = 0  # evaluations that started above the streaming order on the strength of a prediction
        self.n_extended = 0         # evaluations that ran in the extended order
        self.n_timeout_retries = 0  # evaluations repeated behind a device time-out (the engine switched to the shared-device mode)
        self._phi_diag = None

    # ------------------------------------------------------------------ internals
    def _allreduce(self, buf):
        if self.world > 1:
            dist.all_reduce(buf, group=self.group)
            self.n_collectives += 1
        return buf

    def _allreduce_stats(self, stats, M):
        """THE exchange of an evaluation: Phi is symmetric, so only [lower triangle | b | yy | kappa] travels
        (4.2 MB instead of 8.4 MB at M = 1024); unpacking mirrors.  ``n_collectives`` counts what was issued."""
        if self.world > 1:
            e = self.engine
            if hasattr(e, "pack_lower"):
                tri = e.pack_lower(stats, M)
                dist.all_reduce(tri, group=self.group)
                e.unpack_lower(tri, M, stats)
            else:
                dist.all_reduce(stats, group=self.group)
            self.n_collectives += 1
        return stats

    def _fetch(self, att, plan, full=True):
        """The one host round trip of an evaluation: a single device-to-host copy of the attempt's result buffer ([out | status word | ... |
        packed gradient], see ``HipEngine.result_buffer``) -- no cast / concatenate launches.  full: with the gradient pass 2 wrote."""
        # (with the correction's slots the whole buffer: they sit at its end)
        upto = att.head if not (full and plan.with_grad) else (None if plan.lo_slots else att.head + plan.nh + 1)
        att.host = host = (att.buf if upto is None else att.buf[:upto]).detach().to("cpu")
        att.o, att.status = self.engine.read_result(host)
        if att.status < 0:  # not a pivot index: the evaluation itself failed (time-out), with raise_on_fail or without
            raise SgpTimeoutError()
        att.complete = (full or not plan.with_grad) and not plan.want_factors
        return att

    @staticmethod
    def _failed(info, raise_on_fail=True):
        """What value / value_and_grad / factors answer to a non-positive Cholesky pivot: the error, or (NaN, the pivot's index)."""
        if raise_on_fail:
            raise NotPositiveDefiniteError(info)
        return float("nan"), {"info": info}

    def _prep_Z(self, Z):
        if Z.dim() == 1:
            Z = Z[:, None]
        return Z.detach().to(dtype=torch.float64, device=self.engine.device).contiguous()

    def _kept_block(self, M, name, make, bytes_per):
        """The block of the local shard's K'_fu shape that the bound keeps in `name` (None: not with this engine, or beyond the budget)."""
        e, n_local = self.engine, int(self.X.shape[0])
        need = ((max(n_local, 1) + 255) // 256 * 256) * ((M + 127) // 128 * 128)
        if not hasattr(e, make) or need * bytes_per > self.kfu_budget_bytes:
            return None
        if getattr(self, name) is None or getattr(self, name).numel() < need:
            setattr(self, name, getattr(e, make)(n_local, M))
        return getattr(self, name)

    def _kfu_for(self, M):
        return self._kept_block(M, "_kfu", "kfu_buffer", 8)

    def _kfu_f16_for(self, M):
        """The fp16 image of K'_fu beside the fp64 block (the extended order's trailing-word product reads it; written by the assembly
        kernel, which spares sgp_suffstats_bwd_lo a conversion pass over the fp64 block: 2.0 of 4.6 ms at C5)."""
        return self._kept_block(M, "_kfu_f16", "kfu_f16_buffer", 10)

    # ------------------------------------------------------------------ single-launch path (small problems)
    def _small_ok(self, M, want_gz=False, sf2=1.0):
        """One cooperative launch instead of ~60: M <= 128, this rank holds all rows, and the caller did not insist on the
        streaming order (the launch evaluates the whitened / PyMC3 order).  Stationary kernels d <= 24; composite kernels
        d <= 8, without dF/dZ (that goes through the materialised path) and with the block's own amplitudes (sf2 = 1)."""
        e = self.engine
        if self.kernel == "composite" and (want_gz or float(sf2) != 1.0):
            return False
        return (self.fused and self.world == 1 and self.form != "streaming" and hasattr(e, "small_eval")
                and e.small_supported(int(self.X.shape[0]), int(M), self.d, self.kernel))

    def _small_eval(self, Z, theta_host, mode, want_grad, want_gz, composite=None):
        """theta_host: the launch's hyper-parameter vector (d + 2 floats; composite kernels: block + [s2], or the log free
        parameters + [log sigma]).  Returns (host out, info, gZ device tensor or None): one launch, one small host-to-device
        copy before it and one device-to-host copy after it; out = [value | gradients (len(theta_host)) | logmarg | trace]."""
        e = self.engine
        nt = len(theta_host)
        if self._small is None or self._small[0].numel() != nt:
            pin = e.device.type == "cuda"
            host = torch.empty(nt, dtype=torch.float64, pin_memory=pin)
            self._small = (host, torch.empty(nt, dtype=torch.float64, device=e.device), e.small_result(nt - 2)[0], host.numpy())
        host, dev_theta, buf, host_np = self._small
        host_np[:] = theta_host  # one vectorised store into the pinned buffer (element-wise tensor stores cost ~1.5 us each)
        dev_theta.copy_(host, non_blocking=True)
        kw = {"composite": composite} if composite is not None else {}
        out, gz, _ = e.small_eval(self.X, self.y, Z, dev_theta, self.jitter, self.kernel, mode=mode, want_grad=want_grad,
                                  want_gz=want_gz, out=buf, **kw)
        h = out.detach().to("cpu")
        info = int(h.numpy()[nt + 3:nt + 4].view("int32")[0])
        if info < 0:
            if hasattr(e, "small_reset"):
                e.small_reset()
            raise SgpTimeoutError()
        return h, info, gz

    def _whitened(self, M):
        if self.form == "auto":
            return hasattr(self.engine, "suffstats_whitened") and self._rows_for_form * int(M) <= self.WHITENED_MAX_WORK
        return self.form == "whitened"

    def _side_state(self, M):
        """(side stream, (z_ready, ready) events, (Kuu, L^-1) buffers for M inducing points) of the two-stream path.  One side stream per
        engine, shared by every bound built on it; events and buffers are this bound's."""
        e = self.engine
        if self._side is None:
            if getattr(e, "_side_stream", None) is None:
                e._side_stream = torch.cuda.Stream(device=e.device, priority=-1)  # ahead of queued pass-1 workgroups
            self._side = (e._side_stream, (torch.cuda.Event(), torch.cuda.Event()), {})
        bufs = self._side[2].get(M)
        if bufs is None:
            self._side[2].clear()  # (one M at a time: a bound whose inducing set changes size does not keep every size)
            bufs = self._side[2][M] = (e.empty(M, M), e.empty(e.lib.sgp_kuu_factor_len(M)))
        return self._side[0], self._side[1], bufs

    def _trace_buf(self):
        if getattr(self, "_trace", None) is None:  # tr(Kuu^-1) + its scratch: one buffer per bound, reused by every evaluation
            self._trace = self.engine.empty(self.engine.lib.sgp_kuu_inverse_trace_len() if hasattr(self.engine, "lib") else 2)
        return self._trace

    _prefer_whitened = property(lambda self: self.guard.open, lambda self, v: setattr(self.guard, "open", bool(v)))  # `guard.open` under its old name

    def _guard_on(self, M):
        """The guard watches this bound: form="auto" above the size where "auto" means whitened anyway, a tolerance, an engine that reports."""
        return self.form == "auto" and self.streaming_tol > 0.0 and hasattr(self.engine, "streaming_error_report") and not self._whitened(M)

    def _extended_ok(self, M):
        """The extended order exists for this bound (a rank-invariant statement: the shard size is the largest one of the job)."""
        e = self.engine
        return (hasattr(e, "suffstats_extended") and self.kernel != "composite" and self.extended_range > 1.0
                and self._rows_for_form * int(M) >= self.whitened_rows_min_work)

    def _bwd_lo_ok(self, M):
        """Pass 2 of the extended order can apply the trailing word of the double-double Phibar here (RBF, K'_fu kept): a
        rank-invariant statement, like `_extended_ok`."""
        e = self.engine
        return (self.extended_dd_phibar and self.extended_lo and hasattr(e, "suffstats_bwd_lo") and hasattr(e, "phibar_dd")
                and e.bwd_lo_supported(self._rows_for_form, int(M), self.d, self.kernel)
                and ((self._rows_for_form + 255) // 256 * 256) * ((int(M) + 127) // 128 * 128) * 8 <= self.kfu_budget_bytes)

    def _plan(self, M, d, with_grad=False, want_gz=False, want_factors=False, grad_reach=None, strict=False):
        """Everything one evaluation settles before its first attempt.  All of it follows from replicated numbers: ranks plan alike."""
        e, p = self.engine, Plan()
        p.M, p.with_grad, p.want_gz, p.want_factors, p.strict = M, with_grad, want_gz, want_factors, strict
        p.guard, p.ext_ok, p.want_lo = self._guard_on(M), self._extended_ok(M), grad_reach is None   # (the sampler mode takes tier 1's gradient as it is)
        lo_ok = with_grad and self._bwd_lo_ok(M)
        p.reach = self.extended_range
        if with_grad:   # (how far the extended order's gradient holds 1e-6: further with both words of its double-double Phibar)
            p.reach = float(grad_reach) if grad_reach is not None else (self.extended_grad_range_lo if lo_ok else self.extended_grad_range)
        if p.guard:
            p.tier = self.guard.start_tier(self.streaming_tol, p.reach, p.ext_ok)
            if strict and p.tier == TIER_WHITENED:
                # strict: the ACCEPTED tier is the one the evaluation's own exact estimate names.  The whitened order states only an upper
                # bound -- whether it would be left for a lower tier was a matter of the guard's memory (the same theta accepted
                # in tier 1 on a fresh bound and in tier 2 after some history).  So a strict evaluation starts at most in the highest tier
                # that states its exact estimate, and reaches the whitened order only when that estimate sends it there.
                p.tier = TIER_EXTENDED if p.ext_ok else TIER_STREAMING
            if p.tier != TIER_STREAMING:
                self.n_direct_whitened += 1
        else:
            p.tier = TIER_EXTENDED if self.form == "extended" else (TIER_WHITENED if self._whitened(M) else TIER_STREAMING)
        p.nh = (e.hyper_len(self.kernel, d) if hasattr(e, "hyper_len") else d) if with_grad else 0
        # (behind the packed gradient: d + 1 slots for the trailing word's correction, which decides whether the explicit pass 2 is trusted)
        p.lo_slots = (p.nh + 1) if (p.guard and p.ext_ok and lo_ok) else 0
        p.extra = p.nh + 1 + (M * d if want_gz else 0) + p.lo_slots if with_grad else 0
        p.lo_check = bool(p.lo_slots) and p.want_lo   # an extended-order gradient is accepted by its trailing-word correction (`_verdict`)
        if p.guard and with_grad and p.tier == TIER_EXTENDED and p.want_lo and self._lo_skip > 0:
            # the trailing word's correction was too large a moment ago: the next few gradient evaluations go straight to the whitened order (no
            # wasted attempt per leapfrog); the pause doubles with every rejection in a row (8, 16, 32) and ends with the first acceptance
            self._lo_skip -= 1
            p.tier = TIER_WHITENED
        # Small shards: pass 2 is enqueued straight behind the tail and ONE copy at the very end brings back F, the status and the
        # gradient -- a failed factorization or a guard repeat then costs a wasted pass 2, which is cheaper than idling the GPU for
        # a host round trip on every leapfrog.  Big shards check first.  The rule is the job's (largest shard), not this rank's:
        # ranks must issue the same collectives in the same order.
        p.early = with_grad and self._rows_for_form * M >= self.early_check_min_work
        return p

    def _kuu_chain(self, Z, ls, sf2, result, trace, factor=True, side=None):
        """(K_uu, L^-1) by engine.kuu + engine.kuu_factor (factor=False: K_uu alone, the tail factors it), on the calling stream -- or, `side`
        (`_side_state`), on the side stream into the bound's buffers: the caller puts the main stream behind `ready` before the chain is read."""
        e = self.engine
        if side is None:
            Kuu = e.kuu(Z, ls, sf2, self.jitter, self.kernel)
            return Kuu, (e.kuu_factor(Kuu, info=result[2], trace_out=trace)[0] if factor else None)
        stream, (z_ready, ready), (Kuu, linv) = side
        z_ready.record(torch.cuda.current_stream(e.device))  # Z is materialised on the main stream
        stream.wait_event(z_ready)
        # (the side stream's accesses to the result buffer and to Kuubar end before events the main stream waits for ahead of its
        # own last use: no record_stream -- the allocator's per-block event bookkeeping costs the host ~25 us per evaluation)
        e.kuu(Z, ls, sf2, self.jitter, self.kernel, out=Kuu, stream=stream)
        e.kuu_factor(Kuu, info=result[2], trace_out=trace, out=linv, stream=stream)  # the evaluation's status word starts as the Kuu status
        ready.record(stream)
        return Kuu, linv

    def _report(self, att, diag, stride, sf2, s2, M):   # the streaming-order estimate and its bound into the attempt's result buffer
        self.engine.streaming_error_report(diag, stride, self._trace_buf(), sf2, s2, self.N, M, (att.buf, att.out, att.info))
        att.reported = True

    def _attempt_streaming(self, Z, ls, sf2, s2, plan):
        """An attempt in tier 0: pass 1, the exchange, the tail -- everything enqueued, nothing read back (as in every tier)."""
        e, M = self.engine, plan.M
        result = e.result_buffer(plan.extra)  # (buf, out, info): everything the host reads back, one allocation
        kfu = self._kfu_for(M) if plan.with_grad else None
        factor = hasattr(e, "kuu_factor")
        trace = self._trace_buf() if plan.guard and factor else None
        # a second stream only pays once pass 1 is long enough to hide the Kuu chain under it (C3-sized and up; at C1 / C2 sizes
        # the hand-over costs more than the 0.1 ms it could hide)
        side = gate = None
        if self.overlap_tail and factor and e.device.type == "cuda" and int(self.X.shape[0]) * M >= self.overlap_min_work:
            # chol(Kuu), its inverse, the conditioning gate and tr(Kuu^-1) depend on (Z, theta) only: engine.kuu + engine.kuu_factor, SIX
            # launches since round 5 (the factorization's launch forms L^-1 itself), on a side stream beside pass 1.  The calling thread
            # enqueues them first (~25 us; through round 4 the chain was ~50 launches, replayed from a hipGraph by a helper thread whose
            # wake-up alone cost 70 us: profiles/r05_v2_c3_timeline.txt), into buffers the bound keeps (no allocation, no stream
            # bookkeeping per evaluation: the previous evaluation's readers are ahead of `z_ready` in the main stream's order).
            side = self._side_state(M)
            Kuu, linv = self._kuu_chain(Z, ls, sf2, result, trace, side=side)
            # Big shards contract on the integer matrix cores, beside which nothing co-schedules: the contraction is gated on the
            # chain's end, so the chain runs beside kernel assembly (only where assembly outlasts the chain -- 2.0 ms vs 0.6 at
            # N = 1M, M = 1024, but 0.3 vs 0.6 at an eighth of it, where gating costs 0.1 ms: rows >= 300 M) ... and only where the
            # integer cores will actually contract (the library's own rule for this engine's context)
            if (hasattr(e, "would_use_i8") and self.kernel != "composite" and int(self.X.shape[0]) >= 300 * M
                    and e.would_use_i8(int(self.X.shape[0]), M)):
                gate = side[1][1]
        try:
            packed = e.suffstats(self.X, self.y, Z, ls, sf2, self.kernel, kfu=kfu, **({"gate": gate} if gate is not None else {}))
            self._allreduce_stats(packed, M)
        finally:
            # the side stream writes `result`, the trace buffer and (Kuu, L^-1) with no record_stream: the main stream must be behind
            # `ready` before any of them can go back to its allocator pool -- also when pass 1 or the exchange raises
            if side is not None:
                torch.cuda.current_stream(e.device).wait_event(side[1][1])
        if side is None:   # one stream: the chain behind pass 1 (without a guard: K_uu alone, the tail factors it itself)
            Kuu, linv = self._kuu_chain(Z, ls, sf2, result, trace, factor=plan.guard and factor)
        res = e.bound(Kuu, packed, s2, self.N, with_adjoints=plan.with_grad, want_factors=plan.want_factors, kuu_linv=linv, result=result)
        att = Attempt(TIER_STREAMING, res, result[0].numel() - plan.extra, packed, Kuu, linv, kfu=kfu)
        if trace is not None:
            self._report(att, packed, M + 1, sf2, s2, M)
        return att

    def _attempt_extended(self, Z, ls, sf2, s2, plan):
        """An attempt in tier 1, the extended streaming order: the whitened statistics from ONE integer-core contraction (39 digit pairs,
        double-double fold) and a double-double triple product; pass 2 from the explicit Phibar on the fp64 K'_fu kept here."""
        e, M, grad, report = self.engine, plan.M, plan.with_grad, plan.guard
        result = e.result_buffer(plan.extra)
        self.n_extended += 1
        Kuu, linv = self._kuu_chain(Z, ls, sf2, result, self._trace_buf() if report else None)
        kfu = self._kfu_for(M) if grad else None
        if report and (self._phi_diag is None or self._phi_diag.numel() < M):
            self._phi_diag = e.empty(M)
        diag = self._phi_diag if report else None
        dd = grad and self.extended_dd_phibar and hasattr(e, "phibar_dd")
        lo = dd and plan.want_lo and kfu is not None and self._bwd_lo_ok(M)
        kfu_f16 = self._kfu_f16_for(M) if lo else None
        packed = e.suffstats_extended(self.X, self.y, Z, ls, sf2, linv, self.kernel, kfu=kfu, level=self.extended_level,
                                      **({"phi_diag": diag} if diag is not None else {}), **({"kfu_f16": kfu_f16} if kfu_f16 is not None else {}))
        self._allreduce_stats(packed, M)
        # pass 2 of this order takes the explicit Phibar = L^-T C L^-1 / (2 s2); formed by two fp64 products its own rounding
        # (eps |L^-T| |C| |L^-1| >> eps |Phibar|) is what limits the gradients -- formed in double-double from the whitened core C the
        # bound returns they are 5-15 x closer (tests/studies/explicit_phibar_pass2.py; +1.3 ms at M = 1024)
        res = e.bound(Kuu, packed, s2, self.N, with_adjoints=grad, want_factors=plan.want_factors, kuu_linv=linv,
                      result=result, whitened=True, **({"want_cw": True} if dd else {}))
        att = Attempt(TIER_EXTENDED, res, result[0].numel() - plan.extra, packed, Kuu, linv, kfu=kfu, kfu_f16=kfu_f16)
        if dd:
            # ... and 35-700 x closer with the trailing word applied as well: an fp16 product K' Phibar_lo beside the fp64 one (_pass2)
            att.Phibar, att.Phibar_lo = e.phibar_dd(att.Cw, linv, s2, want_lo=lo)
        if report:
            self._allreduce(diag[:M])  # (ranks hold the diagonal of their own shard's Phi)
            self._report(att, diag, 1, sf2, s2, M)
        return att

    def _attempt_whitened(self, Z, ls, sf2, s2, plan):
        """An attempt in tier 2, PyMC3's op order: chol(Kuu) first, then A = L^-1 K_uf, W = A A^T (one stream; these shards are small)."""
        e, M = self.engine, plan.M
        result = e.result_buffer(plan.extra)
        report = plan.guard and self.kernel != "composite"
        Kuu, linv = self._kuu_chain(Z, ls, sf2, result, self._trace_buf() if report else None)
        # with adjoints: also the whitened core Cw of Phibar, so that pass 2 applies L^-T Cw L^-1 factor by factor
        factored = plan.with_grad and self.factored_adjoint and hasattr(e, "suffstats_bwd_factored")
        t_keep = None
        if whitened_rows_layout(e, self.kernel, int(self.X.shape[0]), M, self.whitened_rows_min_work):
            # a large shard (the streaming guard's repeats at 10^6 rows): the streaming layout; T = K'_fu L^-T stays for pass 2
            t_keep = self._kfu_for(M) if factored else None
            packed = e.suffstats_whitened_rows(self.X, self.y, Z, ls, sf2, linv, self.kernel, t_out=t_keep)
        else:
            packed = e.suffstats_whitened(self.X, self.y, Z, ls, sf2, linv, self.kernel)
        self._allreduce_stats(packed, M)
        res = e.bound(Kuu, packed, s2, self.N, with_adjoints=plan.with_grad, want_factors=plan.want_factors, kuu_linv=linv,
                      result=result, whitened=True, **({"want_cw": True} if factored else {}))
        att = Attempt(TIER_WHITENED, res, result[0].numel() - plan.extra, packed, Kuu, linv, t_keep=t_keep, factored=res.get("Cw") is not None)
        if report:
            self._report(att, None, 1, sf2, s2, M)
        return att

    def _pass2(self, att, Z, ls, sf2, s2, plan):
        """Pass 2 on the local rows + the all-reduce of the gradients + the K_uu path, into the packed gradient behind the attempt's head."""
        e, g, n_lo = self.engine, att.buf[att.head:], plan.lo_slots
        kappabar = -1.0 / (2.0 * float(s2))   # dF/dkappa needs nothing from the device (same value the tail writes to out)
        if att.factored:
            # whitened order: Phibar's cond(K_uu)-sized entries would cancel in Phibar K_uf -- its factors are applied instead
            e.suffstats_bwd_factored(self.X, self.y, Z, ls, sf2, att.linv, att.Cw, s2, att.bbar, kappabar, self.kernel,
                                     want_gz=plan.want_gz, out=g, **({"t_in": att.t_keep} if att.t_keep is not None else {}))
        else:
            e.suffstats_bwd(self.X, self.y, Z, ls, sf2, att.Phibar, att.bbar, kappabar, self.kernel, want_gz=plan.want_gz, out=g, kfu=att.kfu)
            if att.Phibar_lo is not None:   # the extended order: the trailing word of its double-double Phibar (lengthscales, amplitude)
                # (the correction itself goes to the tail of `g`: all-reduced with it, read back with it)
                e.suffstats_bwd_lo(self.X, self.y, Z, ls, sf2, att.Phibar_lo, att.kfu, g, self.kernel,
                                   **({"delta": g[g.numel() - n_lo:]} if n_lo else {}),
                                   **({"kfu_f16": att.kfu_f16} if att.kfu_f16 is not None else {}))
        if n_lo and att.Phibar_lo is None:
            g[g.numel() - n_lo:].zero_()   # (the correction's slots travel with g: nothing undefined into the all-reduce)
        self._allreduce(g)
        # (measured and dropped, round 5: this launch pair on the side stream beside pass 2 -- it needs Kuubar only -- ends the evaluation no
        # earlier: pass 2 fills the chip and runs the 28 us longer that the side stream takes from it, profiles/r05_kuu_bwd_side_stream_c3_timeline.txt)
        e.kuu_bwd(Z, ls, sf2, att.Kuubar, g, self.kernel, want_gz=plan.want_gz)

    def _lo_correction_small(self, att, plan):
        """The a-posteriori check of the extended order's gradient: the trailing word's correction [d lengthscales | sf2] (tail of the
        buffer) against the gradient it went into, in the parity suite's metric -- lengthscales against their largest component,
        the amplitude against max(1, |g_sf2|)."""
        host, nh = att.host, plan.nh
        g, dl = host[att.head:att.head + nh + 1].tolist(), host[host.numel() - plan.lo_slots:].tolist()
        if any(v != v for v in dl):   # NaN: the product's inputs were beyond its fp16 format (an inducing point > 128 lengthscales out) -- no correction was added
            self.last_lo_correction = float("inf")
            return False
        self.last_lo_correction = max(max(abs(v) for v in dl[:nh]) / max(1.0, max(abs(v) for v in g[:nh])), abs(dl[nh]) / max(1.0, abs(g[nh])))
        return self.last_lo_correction <= self.extended_lo_max_correction

    def _verdict(self, att, plan, may_go_down):
        """What a fetched attempt's own numbers say: None = accept, or the tier to repeat the evaluation in.  The ONE place that reads the
        estimate and the bound and updates what the guard remembers -- once per attempt, however often it is asked.
        A failed factorization of K_uu (status in 1 .. M) or a refusal says nothing about the estimate: the state is left alone and
        nothing is repeated.  A failed factorization of B (status > M) below the whitened order is the streaming order's own failure
        mode -- W = L^-1 Phi L^-T so far off that I + W / s2 is not positive definite (l = 20, sig_n = 0.01: profiles/r04_theta_sweep_streaming.jsonl)
        -- and the estimate, which needs K_uu's factor and Phi only, is valid: it is reviewed like any other."""
        tier, status = att.tier, att.status
        if plan.guard and att.reported and (status == 0 or (status > plan.M and tier < TIER_WHITENED)):
            if att.need is None:
                e, tol = self.engine, self.streaming_tol
                est, ub = e.read_estimate(att.host), e.read_bound(att.host)
                self.last_estimate = est
                if tier == TIER_WHITENED:
                    # (only the upper bound is known here: nothing this order states can send the evaluation DOWN -- a strict evaluation never
                    # starts in it, see _plan, so whatever is accepted here was sent up by a lower tier's exact estimate)
                    self.guard.note_bound(ub, tol)
                    att.need = tier
                else:
                    att.need = required_tier(est, tol, plan.reach, plan.ext_ok)
                    self.guard.note_exact(est, ub, tol)
                    if att.need > tier:
                        self.guard.open = True
            if att.need > tier:
                return att.need
            if status != 0:  # B failed although the estimate is inside this tier's reach: the next tier up, if there is one
                return tier + 1 if (tier + 1 < TIER_WHITENED and plan.ext_ok) else TIER_WHITENED
            if may_go_down and att.need < tier:
                return att.need
        if plan.lo_check and tier == TIER_EXTENDED and att.Phibar_lo is not None and (att.complete or status != 0):
            if status == 0 and not self._lo_correction_small(att, plan):
                # The explicit pass 2 of this order is trusted only while its trailing-word correction is small against the gradient (what is
                # left behind the correction is a few per cent of it: profiles/r06_extended_order_gradients_*): repeated in the whitened order
                self.n_lo_rejections += 1
                self._lo_pause = min(32, 2 * self._lo_pause) if self._lo_pause else 8
                self._lo_skip = self._lo_pause
                return TIER_WHITENED
            self._lo_pause = 0   # accepted: the next rejection starts with the short pause again
        return None

    def _evaluate(self, *args, **kw):
        """`_walk`, and ONE more attempt behind a device time-out: the single-launch Cholesky deals its work items statically and needs all its
        workgroups resident (the fast way while this process has the GPU to itself); a second process on the same device -- joblib workers as
        in the reference's experiments/regression.py:219-231 -- can starve such a launch into SGP_INFO_TIMEOUT.  The first time-out switches this
        engine's context to SGP_OPT_SHARED_DEVICE (items claimed by ticket, by workgroups that are running: include/sgp.h) for good and the
        evaluation is repeated; a second time-out is raised.  With ONE rank only: the status word is per rank (never all-reduced), so a rank
        repeating on its own would pair its collectives with the other ranks' NEXT evaluation -- they raise at once, as before round 6."""
        try:
            return self._walk(*args, **kw)
        except SgpTimeoutError:
            e = self.engine
            if self.world > 1 or "shared_device" not in getattr(e, "OPTIONS", {}) or e.get_option("shared_device") != 0:
                raise
            e.set_option("shared_device", 1)
            self.n_timeout_retries += 1
            return self._walk(*args, **kw)

    def _walk(self, Z, ls, sf2, s2, **request):
        """ONE evaluation through the guard -- the driver value / value_and_grad / factors share (`request`: see `_plan`).  Runs attempts
        until `_verdict` accepts one and returns it (with_grad: the packed gradient sits behind its `head`, on the host and in `buf`)."""
        plan = self._plan(int(Z.shape[0]), int(Z.shape[1]), **request)
        # Repeats: UP whenever the attempt's own estimate asks for a higher tier; DOWN (strict only) at most once, and never again after
        # it -- so the walk ends after at most four attempts (1 -> 0 -> 1 -> 2) and what is accepted is never an attempt whose own estimate
        # asked for more (`nxt in tried` used to fall through to the LOWER attempt).  Attempts that are complete (everything
        # already on the host) are kept, so coming back to a tier costs nothing; an incomplete one (big shards: pass 2 not yet run, and
        # its K'_fu buffer since overwritten) is run again.
        done, tier, may_go_down = {}, plan.tier, plan.strict
        while True:
            att = done.get(tier)   # (a kept attempt passes the same verdict as a fresh one; the guard's memory saw it once: `need`)
            if att is None:
                att = (self._attempt_streaming, self._attempt_extended, self._attempt_whitened)[tier](Z, ls, sf2, s2, plan)
                if plan.with_grad and not plan.early:
                    self._pass2(att, Z, ls, sf2, s2, plan)
                self._fetch(att, plan, full=not plan.early)
            nxt = self._verdict(att, plan, may_go_down)
            if nxt is None and not att.complete and plan.early and att.status == 0:   # big shards: the status was read first, pass 2 goes behind an accepted tail
                self._pass2(att, Z, ls, sf2, s2, plan)
                self._fetch(att, plan, full=True)
                nxt = self._verdict(att, plan, may_go_down)
            if nxt is None:
                break
            if att.complete:
                done[tier] = att
            if nxt < tier:
                may_go_down = False
            self.n_guard_reruns += 1
            tier = nxt
        self.last_tier = tier
        return att

    # ------------------------------------------------------------------ public
    def value(self, Z, ls, sf2, s2, raise_on_fail=True, strict=False):
        """F (not divided by N).  Returns (F, parts) with parts = dict(logmarg, trace_term, info)."""
        Z = self._prep_Z(Z)
        if self._small_ok(Z.shape[0], sf2=sf2):
            th, comp = self._natural_theta(ls, sf2, s2)
            nh = len(th) - 1
            h, info, _ = self._small_eval(Z, th, 0, False, False, comp)
            self.n_evals += 1
            if info != 0:
                return self._failed(info, raise_on_fail)
            hl = h.tolist()  # (plain floats once: indexing the tensor costs ~1.5 us per element)
            return hl[0], {"logmarg": hl[nh + 2], "trace_term": hl[nh + 3], "info": 0}
        att = self._evaluate(Z, ls, sf2, s2, strict=strict)
        self.n_evals += 1
        if att.status != 0:
            return self._failed(att.status, raise_on_fail)
        return float(att.o[OUT_F]), {"logmarg": float(att.o[OUT_LOGMARG]), "trace_term": float(att.o[OUT_TRACE]), "info": 0}

    def _natural_theta(self, ls, sf2, s2):
        """(theta of the single launch in natural parameters, composite description or None)."""
        vals = [float(v) for v in (ls.tolist() if hasattr(ls, "tolist") else ls)]
        if self.kernel == "composite":
            if len(vals) != COMP_LEN:
                raise ValueError("composite kernels take the %d-entry parameter block as `ls`" % COMP_LEN)
            return vals + [float(s2)], {"structure": vals}
        if len(vals) == 1 and self.d > 1:
            vals = vals * self.d
        if len(vals) != self.d:
            raise ValueError("lengthscale has %d entries, expected %d" % (len(vals), self.d))
        return vals + [float(sf2), float(s2)], None

    def value_and_grad(self, Z, ls, sf2, s2, want_gz=False, raise_on_fail=True, grad_reach=None, strict=False):
        """F and dF/d{lengthscale_j, sf2, s2[, Z]} (natural parameters, not their raw transforms).

        Returns (F, grads) with grads = dict(ls=tensor[d] (cpu), sf2=float, s2=float, Z=device tensor or None).
        grad_reach / strict: see HmcTarget(gradient="sampler") -- how far (x the tolerance) the extended order's explicit-Phibar gradient
        is accepted (default: `extended_grad_range`, what keeps 1e-6), and whether the accepted tier must be the one the evaluation's own
        estimate names (so that value and gradient are functions of theta alone).
        """
        e = self.engine
        Z = self._prep_Z(Z)
        M, d = Z.shape
        if self._small_ok(M, want_gz, sf2):
            th, comp = self._natural_theta(ls, sf2, s2)
            h, info, gz = self._small_eval(Z, th, 0, True, want_gz, comp)
            self.n_evals += 1
            self.n_grads += 1
            if info != 0:
                return self._failed(info, raise_on_fail)
            nh = len(th) - 1  # kernel hyper-parameter entries: d lengthscales + sf2, or the composite block
            hl = h.tolist()
            if comp is not None:
                return hl[0], {"ls": h[1:1 + nh].clone(), "sf2": 0.0, "s2": hl[1 + nh], "Z": None, "info": 0,
                               "logmarg": hl[nh + 2], "trace_term": hl[nh + 3]}
            return hl[0], {"ls": h[1:1 + d].clone(), "sf2": hl[1 + d], "s2": hl[2 + d], "Z": gz, "info": 0,
                           "logmarg": hl[d + 3], "trace_term": hl[d + 4]}
        nh = e.hyper_len(self.kernel, d) if hasattr(e, "hyper_len") else d  # composite kernels: the parameter block
        att = self._evaluate(Z, ls, sf2, s2, with_grad=True, want_gz=want_gz, grad_reach=grad_reach, strict=strict)
        self.n_evals += 1
        self.n_grads += 1
        if att.status != 0:
            return self._failed(att.status, raise_on_fail)
        o, gh, g = att.o, att.host[att.head:], att.buf[att.head:]
        grads = {"ls": gh[:nh].clone(), "sf2": float(gh[nh]), "s2": float(o[OUT_S2BAR]),
                 "Z": g[nh + 1:nh + 1 + M * d].reshape(M, d) if want_gz else None, "info": 0,
                 "logmarg": float(o[OUT_LOGMARG]), "trace_term": float(o[OUT_TRACE])}
        return float(o[OUT_F]), grads

    def factors(self, Z, ls, sf2, s2):
        """Device tensor [Linv | G | q] for ``predict`` (computed from the current statistics)."""
        Z = self._prep_Z(Z)
        att = self._evaluate(Z, ls, sf2, s2, want_factors=True)
        if att.status != 0:
            self._failed(att.status)
        return att.factors

    def predict(self, Xs, Z, ls, sf2, s2, pred_noise=True, full_cov=False, factors=None):
        """Posterior predictive mean / variance (/ covariance) at Xs -- models/sgpr.py:150-160, 256-286."""
        Z = self._prep_Z(Z)
        if Xs.dim() == 1:
            Xs = Xs[:, None]
        Xs = Xs.detach().to(dtype=torch.float64, device=self.engine.device).contiguous()
        if factors is None:
            factors = self.factors(Z, ls, sf2, s2)
        return self.engine.predict(Xs, Z, ls, sf2, s2, factors, self.kernel, pred_noise=pred_noise, full_cov=full_cov)


def device_run_fits(n_rows: int, n_draws_total: int, max_treedepth: int) -> bool:
    """sgp_small_nuts refuses (SGP_ERR_DIM) a run whose worst case -- (draws + 2) x 2^depth evaluations x workgroups of the launch
    (3 + one per 64-row slab, at most 211) -- could pass 2^31, the range of its cumulative sync counters."""
    grid = 3 + min((int(n_rows) + 63) // 64, 208)
    return (float(n_draws_total) + 2.0) * float(1 << int(max_treedepth)) * grid <= 2.0e9


def shard_rows(N: int, rank: int, world: int):
    """Contiguous row block [lo, hi) of rank ``rank`` (X[g N/G : (g+1) N/G])."""
    base, rem = divmod(N, world)
    lo = rank * base + min(rank, rem)
    hi = lo + base + (1 if rank < rem else 0)
    return lo, hi
