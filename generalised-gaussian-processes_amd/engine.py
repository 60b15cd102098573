"""HipEngine: torch-tensor front end of the C ABI (include/sgp.h).

PyTorch is plumbing here: it owns device memory, the current HIP stream and (in ``core``) the
RCCL process group.  All arithmetic happens inside libsgp_hip.so.  Every method takes / returns
fp64 CUDA(=HIP) tensors; hyper-parameters are host floats (they travel as kernel arguments).

The engine interface (``suffstats`` / ``bound`` / ``suffstats_bwd`` / ``kuu_bwd`` / ``predict``) is
the seam the CPU-only tests use to exercise the host logic above it with a test double; the product
constructs ``HipEngine`` and nothing else.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import COMP_LEN, KERNEL_IDS, OUT_LEN

RESULT_HEAD = OUT_LEN + 4  # doubles ahead of the caller's extras in a result buffer: out, status word, estimate, bound, pad


def _kernel_id(kernel) -> int:
    if isinstance(kernel, int):
        if kernel not in KERNEL_IDS.values():
            raise ValueError("unknown kernel id %r" % (kernel,))
        return kernel
    try:
        return KERNEL_IDS[str(kernel).lower()]
    except KeyError:
        raise ValueError("unknown kernel %r (expected one of %s)" % (kernel, sorted(KERNEL_IDS))) from None


def _likelihood_id(likelihood) -> int:
    """SGP_LIK_* of a likelihood name ("bernoulli" = "bernoulli_probit")."""
    name = "bernoulli" if likelihood == "bernoulli_probit" else likelihood
    if name not in _lib.LIKELIHOOD_IDS:
        raise ValueError("unknown likelihood %r (known: %s)" % (likelihood, ", ".join(sorted(_lib.LIKELIHOOD_IDS))))
    return _lib.LIKELIHOOD_IDS[name]


_F64 = torch.float64


def _chk(device, t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype is not _F64 or t.device != device or not t.is_contiguous():
        raise ValueError("%s must be a contiguous float64 tensor on %s (got %s, %s)" % (name, device, t.dtype, t.device))
    return t


class HipEngine:
    """Calls the HIP library on ``device`` (default: current CUDA device).  No CPU fallback.

    ``own_context=True`` gives the engine a library context of its own (include/sgp.h: sgp_ctx_create): its contraction mode,
    conditioning limit, budgets and timing events are then independent of every other engine in the process (``set_option`` /
    ``get_option`` / ``contraction_last``).  The default engine runs in the library's DEFAULT context -- the one the deprecated
    process-wide setters (``lib.sgp_set_contraction`` ...) act on."""

    OPTIONS = {"contraction": _lib.OPT_CONTRACTION, "asm_overlap": _lib.OPT_ASM_OVERLAP, "kfu_budget_bytes": _lib.OPT_KFU_BUDGET_BYTES,
               "cond_limit": _lib.OPT_COND_LIMIT, "cu_budget": _lib.OPT_CU_BUDGET, "timing": _lib.OPT_TIMING,
               "shared_device": _lib.OPT_SHARED_DEVICE}

    def __init__(self, device: Optional[torch.device] = None, own_context: bool = False):
        self.lib = _lib.load_library()
        if not torch.cuda.is_available():
            raise _lib.SgpLibraryError("HipEngine needs a HIP device (torch.cuda.is_available() is False); "
                                       "there is no CPU implementation of the sparse-GP core")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._ws = {}
        self._ctx = None  # NULL = the default context
        if own_context:
            self._ctx = self.lib.sgp_ctx_create(self.device.index if self.device.index is not None else torch.cuda.current_device())
            if not self._ctx:
                raise _lib.SgpLibraryError("sgp_ctx_create failed")

    def __del__(self):
        ctx, self._ctx = getattr(self, "_ctx", None), None
        if ctx:
            try:
                self.lib.sgp_ctx_destroy(C.c_void_p(ctx))
            except Exception:  # noqa: BLE001 - interpreter shutdown
                pass

    # ------------------------------------------------------------------ context
    class _ContextFree:
        """The entry points that take no context argument (sgp_chol_lower, sgp_predict, the sgp_svgp_* and sgp_small_* families), called
        with this engine's context bound to the calling thread for the duration of the call (include/sgp.h: sgp_ctx_bind_thread), so
        that they read ITS options -- CU budget, conditioning limit, shared-device mode.  An engine on the default context calls straight
        through."""

        def __init__(self, eng):
            self._eng = eng

        def __getattr__(self, name):
            eng = self._eng
            fn = getattr(eng.lib, name)
            if not eng._ctx:
                return fn
            bind = eng.lib.sgp_ctx_bind_thread

            def call(*a):
                bind(C.c_void_p(eng._ctx))
                try:
                    return fn(*a)
                finally:
                    bind(C.c_void_p(0))
            return call

    @property
    def _cf(self):
        cf = self.__dict__.get("_cf_obj")
        if cf is None:
            cf = self.__dict__["_cf_obj"] = HipEngine._ContextFree(self)
        return cf

    def _c(self):
        return C.c_void_p(self._ctx) if self._ctx else C.c_void_p(0)

    def set_option(self, name: str, value) -> float:
        """Sets an option of this engine's context (``OPTIONS``); returns the previous value."""
        prev = self.lib.sgp_ctx_get_option(self._c(), self.OPTIONS[name])
        _lib.check("sgp_ctx_set_option", self.lib.sgp_ctx_set_option(self._c(), self.OPTIONS[name], float(value)))
        return prev

    def get_option(self, name: str) -> float:
        return self.lib.sgp_ctx_get_option(self._c(), self.OPTIONS[name])

    def contraction_last(self) -> int:
        """What this engine's last pass 1 ran: 0 fp64 matrix cores, 1 integer matrix cores."""
        return int(self.lib.sgp_ctx_contraction_last(self._c()))

    def would_use_i8(self, N: int, M: int) -> bool:
        """The contraction rule of this engine's context for an N-row shard with M inducing inputs."""
        return bool(self.lib.sgp_ctx_contraction_would_use_i8(self._c(), int(N), int(M)))

    # ------------------------------------------------------------------ helpers
    def _workspace(self, name: str, nbytes: int) -> torch.Tensor:
        buf = self._ws.get(name)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
            self._ws[name] = buf
        return buf

    def _stream(self, stream=None):
        """The HIP stream handle of `stream` (a torch.cuda.Stream), default torch's current one on this device."""
        return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(self.device)).cuda_stream)

    def _chk(self, t: torch.Tensor, name: str) -> torch.Tensor:
        return _chk(self.device, t, name)

    @staticmethod
    def hyper_len(kernel, d: int) -> int:
        """Entries of the hyper-parameter gradient: d lengthscales, or the composite kernel's parameter block."""
        return COMP_LEN if _kernel_id(kernel) == KERNEL_IDS["composite"] else d

    def _inv_ls(self, ls: Sequence[float], d: int, kernel="rbf"):
        """1 / lengthscale as the C array the entry points take.  An evaluation passes the same list to four or five calls: the last
        array is kept (the library copies it during the call)."""
        c = self.__dict__.get("_ils")
        if c is not None and type(ls) is list and c[1] == d and c[2] == kernel and c[0] == ls:
            return c[3]
        vals = [float(v) for v in (ls.tolist() if hasattr(ls, "tolist") else ls)]
        if _kernel_id(kernel) == KERNEL_IDS["composite"]:  # the parameter block travels in place of 1 / lengthscale
            if len(vals) != COMP_LEN:
                raise ValueError("a composite kernel takes a %d-entry parameter block (got %d)" % (COMP_LEN, len(vals)))
            arr = (C.c_double * COMP_LEN)(*vals)
        else:
            if len(vals) == 1 and d > 1:
                vals = vals * d
            if len(vals) != d:
                raise ValueError("lengthscale has %d entries, expected %d" % (len(vals), d))
            arr = (C.c_double * d)(*[1.0 / v for v in vals])
        if type(ls) is list:
            self._ils = (list(ls), d, kernel, arr)
        return arr

    @staticmethod
    def _ptr(t: Optional[torch.Tensor]):
        return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else C.c_void_p(0)

    def empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float64, device=self.device)

    # ------------------------------------------------------------------ pass 1
    def _pass1(self, X, y, Z, kuu_linv, out, ws_name: str, ws_query, *query_args, limits: str = ""):
        """What the four ``suffstats*`` wrappers share: shapes, tensor checks, the packed ``out``, the workspace (``ws_query`` of this
        engine's context at (N, M, d, *query_args), cached as ``ws_name``) and the four pointers [Phi or W | b or u | yy | kappa] into
        ``out``.  Returns (N, M, d, out, ws, pointers)."""
        N, d = X.shape
        M = Z.shape[0]
        self._chk(Z, "Z")
        if kuu_linv is not None:
            self._chk(kuu_linv, "kuu_linv")
        if N > 0:
            self._chk(X, "X"), self._chk(y, "y")
        if out is None:
            out = self.empty(M * M + M + 2)
        nbytes = ws_query(self._c(), N, M, d, *query_args)
        if nbytes == 0:
            raise ValueError("unsupported shape N=%d M=%d d=%d%s" % (N, M, d, limits))
        base = out.data_ptr()
        stats = [C.c_void_p(base + 8 * o) for o in (0, M * M, M * M + M, M * M + M + 1)]
        return N, M, d, out, self._workspace(ws_name, nbytes), stats

    def kfu_buffer(self, N: int, M: int) -> torch.Tensor:
        """Caller-owned K'_fu block (see include/sgp.h: sgp_kfu_len) for ``suffstats(..., kfu=)``."""
        return self.empty(self.lib.sgp_kfu_len(N, M))

    def kfu_f16_buffer(self, N: int, M: int) -> torch.Tensor:
        """Caller-owned fp16 image of K'_fu (sgp_kfu_len 16-bit words) for ``suffstats_extended(..., kfu_f16=)`` / ``suffstats_bwd_lo(..., kfu_f16=)``."""
        return torch.empty(self.lib.sgp_kfu_len(N, M), dtype=torch.float16, device=self.device)

    def suffstats(self, X, y, Z, ls, sf2, kernel="rbf", out: Optional[torch.Tensor] = None,
                  kfu: Optional[torch.Tensor] = None, gate: Optional[torch.cuda.Event] = None) -> torch.Tensor:
        """Packed local statistics [Phi (M*M) | b (M) | yy | kappa] -- the buffer the all-reduce sums.

        ``kfu`` (optional, from ``kfu_buffer``) keeps the assembled kernel block for ``suffstats_bwd``.  ``gate``: an event
        already recorded on another stream that the integer-core contraction waits for (include/sgp.h: sgp_set_pass1_gate)."""
        # with a caller-owned K'_fu the library's own super-chunk (up to 16 GiB) is not part of the workspace
        N, M, d, out, ws, stats = self._pass1(X, y, Z, None, out, "fwd_kfu" if kfu is not None else "fwd",
                                              self.lib.sgp_ctx_suffstats_workspace_bytes, 1 if kfu is not None else 0,
                                              limits=" (d <= %d, M <= %d)" % (_lib.SGP_MAX_DIM, _lib.SGP_MAX_INDUCING))
        if gate is not None:
            self.lib.sgp_ctx_set_pass1_gate(self._c(), C.c_void_p(gate.cuda_event))
        st = self.lib.sgp_ctx_suffstats_fwd(
            self._c(), self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), N, M, d, _kernel_id(kernel),
            *stats, self._ptr(kfu), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_suffstats_fwd", st)
        return out

    def suffstats_whitened(self, X, y, Z, ls, sf2, kuu_linv, kernel="rbf", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Packed local statistics in the whitened basis, [W = A A^T (M*M) | u = A y (M) | yy | kappa] with A = L^-1 K_uf
        (PyMC3's op order; ``kuu_linv`` from ``kuu_factor``).  Same layout and all-reduce as ``suffstats``."""
        N, M, d, out, ws, stats = self._pass1(X, y, Z, kuu_linv, out, "fwd_whitened", self.lib.sgp_ctx_suffstats_whitened_workspace_bytes)
        st = self.lib.sgp_ctx_suffstats_fwd_whitened(
            self._c(), self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), N, M, d, _kernel_id(kernel),
            self._ptr(kuu_linv), *stats, self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_suffstats_fwd_whitened", st)
        return out

    def suffstats_whitened_rows(self, X, y, Z, ls, sf2, kuu_linv, kernel="rbf", out: Optional[torch.Tensor] = None,
                                t_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``suffstats_whitened`` for a large shard, in the streaming layout (include/sgp.h: sgp_suffstats_fwd_whitened_rows; stationary
        kernels).  ``t_out`` (from ``kfu_buffer``) keeps T = K'_fu L^-T for ``suffstats_bwd_factored(..., t_in=)``."""
        N, M, d, out, ws, stats = self._pass1(X, y, Z, kuu_linv, out, "fwd_whitened_rows_t" if t_out is not None else "fwd_whitened_rows",
                                              self.lib.sgp_ctx_suffstats_whitened_rows_workspace_bytes, 1 if t_out is not None else 0)
        if t_out is not None:
            self._chk(t_out, "t_out")
            if t_out.numel() < self.lib.sgp_kfu_len(N, M):
                raise ValueError("t_out holds %d doubles, sgp_kfu_len(N, M) = %d" % (t_out.numel(), self.lib.sgp_kfu_len(N, M)))
        st = self.lib.sgp_ctx_suffstats_fwd_whitened_rows(
            self._c(), self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), N, M, d, _kernel_id(kernel),
            self._ptr(kuu_linv), *stats, self._ptr(t_out), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_suffstats_fwd_whitened_rows", st)
        return out

    def suffstats_extended(self, X, y, Z, ls, sf2, kuu_linv, kernel="rbf", out: Optional[torch.Tensor] = None,
                           kfu: Optional[torch.Tensor] = None, level: int = 1, phi_diag: Optional[torch.Tensor] = None,
                           kfu_f16: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The whitened statistics [W | u | yy | kappa] from the EXTENDED streaming order (include/sgp.h: sgp_suffstats_fwd_extended):
        Phi on the integer matrix cores to 2^-61, the triple product in double-double.  ``kfu`` (from ``kfu_buffer``) keeps the fp64
        K'_fu for ``suffstats_bwd``.  ``level`` 1: 34 digit pairs (Phi to 2^-61), 2: 39 pairs (2^-69).  Stationary kernels.
        ``phi_diag`` (M doubles): receives diag(K_uf K_fu) of this shard for ``streaming_error_report`` (ranks add theirs up).
        ``kfu_f16`` (from ``kfu_f16_buffer``, with ``kfu``): receives the fp16 image of K'_fu for ``suffstats_bwd_lo``."""
        N, M, d, out, ws, stats = self._pass1(X, y, Z, kuu_linv, out, "fwd_extended", self.lib.sgp_ctx_suffstats_extended_workspace_bytes)
        if kfu is not None:
            self._chk(kfu, "kfu")
            if kfu.numel() < self.lib.sgp_kfu_len(N, M):
                raise ValueError("kfu holds %d doubles, sgp_kfu_len(N, M) = %d" % (kfu.numel(), self.lib.sgp_kfu_len(N, M)))
        if phi_diag is not None:
            self._chk(phi_diag, "phi_diag")
            if phi_diag.numel() < M:
                raise ValueError("phi_diag holds %d doubles, M = %d" % (phi_diag.numel(), M))
        if kfu_f16 is not None:
            if kfu is None or kfu_f16.dtype != torch.float16 or not kfu_f16.is_contiguous() or kfu_f16.device != self.device \
                    or kfu_f16.numel() < self.lib.sgp_kfu_len(N, M):
                raise ValueError("kfu_f16: a contiguous float16 tensor of sgp_kfu_len(N, M) elements on this device, together with kfu")
        st = self.lib.sgp_ctx_suffstats_fwd_extended_f16(
            self._c(), self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), N, M, d, _kernel_id(kernel),
            self._ptr(kuu_linv), int(level), *stats, self._ptr(kfu), self._ptr(kfu_f16), self._ptr(phi_diag), self._ptr(ws), ws.numel(),
            self._stream())
        _lib.check("sgp_suffstats_fwd_extended", st)
        return out

    def phibar_dd(self, Cw: torch.Tensor, kuu_linv: torch.Tensor, s2: float, want_lo: bool = False):
        """Phibar = L^-T (Cw / 2 s2) L^-1 formed in double-double (include/sgp.h: sgp_phibar_dd): (leading word, trailing word or None),
        M x M each.  The leading word replaces the fp64-formed Phibar of ``bound(..., whitened=True)`` in the extended order's pass 2."""
        M = Cw.shape[0]
        self._chk(Cw, "Cw"), self._chk(kuu_linv, "kuu_linv")
        hi = self.empty(M, M)
        lo = self.empty(M, M) if want_lo else None
        ws = self._workspace("phibar_dd", self.lib.sgp_phibar_dd_workspace_bytes(M))
        st = self.lib.sgp_phibar_dd(self._ptr(Cw), self._ptr(kuu_linv), M, float(s2), self._ptr(hi), self._ptr(lo),
                                    self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_phibar_dd", st)
        return hi, lo

    def bwd_lo_supported(self, N: int, M: int, d: int, kernel="rbf") -> bool:
        """``suffstats_bwd_lo`` exists for this shape: RBF (any d the streaming kernels take)."""
        return kernel == "rbf" and self.lib.sgp_suffstats_bwd_lo_workspace_bytes(int(N), int(M), int(d)) > 0

    def suffstats_bwd_lo(self, X, y, Z, ls, sf2, Phibar_lo, kfu, grads: torch.Tensor, kernel="rbf", delta: Optional[torch.Tensor] = None,
                         kfu_f16: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Adds the trailing word's share of pass 2 into the packed gradients ``suffstats_bwd`` wrote (include/sgp.h: sgp_suffstats_bwd_lo);
        ``delta`` (d + 1 doubles) receives the correction itself.  ``kfu_f16``: the fp16 image ``suffstats_extended(..., kfu_f16=)`` left
        (the conversion pass is skipped; ``kfu`` may then be None)."""
        N, d = X.shape
        M = Z.shape[0]
        self._chk(Phibar_lo, "Phibar_lo")
        if kfu is not None:
            self._chk(kfu, "kfu")
        elif kfu_f16 is None:
            raise ValueError("suffstats_bwd_lo needs kfu or kfu_f16")
        if kfu_f16 is not None and (kfu_f16.dtype != torch.float16 or kfu_f16.device != self.device or kfu_f16.numel() < self.lib.sgp_kfu_len(N, M)):
            raise ValueError("kfu_f16: a float16 tensor of sgp_kfu_len(N, M) elements on this device")
        nh = self.hyper_len(kernel, d)
        ws = self._workspace("bwd_lo", self.lib.sgp_suffstats_bwd_lo_workspace_bytes_ex(N, M, d, 1 if kfu_f16 is not None else 0))
        base = grads.data_ptr()
        st = self.lib.sgp_suffstats_bwd_lo_f16(self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2),
                                               self._ptr(Phibar_lo), self._ptr(kfu), self._ptr(kfu_f16), N, M, d, _kernel_id(kernel),
                                               C.c_void_p(base), C.c_void_p(base + 8 * nh), self._ptr(delta), self._ptr(ws), ws.numel(),
                                               self._stream())
        _lib.check("sgp_suffstats_bwd_lo", st)
        return grads

    def pack_lower(self, stats: torch.Tensor, M: int) -> torch.Tensor:
        """[lower triangle of Phi | b | yy | kappa]: what crosses xGMI (half the bytes of ``stats``)."""
        tri = self.empty(self.lib.sgp_stats_packed_len(M))
        _lib.check("sgp_stats_pack_lower", self.lib.sgp_stats_pack_lower(self._ptr(stats), M, self._ptr(tri), self._stream()))
        return tri

    def unpack_lower(self, tri: torch.Tensor, M: int, stats: torch.Tensor) -> torch.Tensor:
        _lib.check("sgp_stats_unpack_lower", self.lib.sgp_stats_unpack_lower(self._ptr(tri), M, self._ptr(stats), self._stream()))
        return stats

    def kuu(self, Z, ls, sf2, jitter, kernel="rbf", out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """K_uu + jitter I.  ``stream``: enqueue there instead of on torch's current stream (the caller orders it against the producers /
        consumers of Z and ``out`` itself)."""
        M, d = Z.shape
        self._chk(Z, "Z")
        K = out if out is not None else self.empty(M, M)
        st = self.lib.sgp_kuu(self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), float(jitter), M, d, _kernel_id(kernel),
                              self._ptr(K), self._stream(stream))
        _lib.check("sgp_kuu", st)
        return K

    # ------------------------------------------------------------------ tail
    def result_buffer(self, extra: int = 0):
        """One allocation for everything the host reads back after an evaluation: (buf, out, info) with
        buf = [out (OUT_LEN doubles) | status word (int32, in the low half of one double) | streaming-order estimate | its upper bound |
               pad | extra doubles]
        (RESULT_HEAD doubles ahead of the extras: they start 16-byte aligned, collectives run on that slice), so a single
        device-to-host copy of ``buf`` -- and no cast / concatenate launches -- ends the evaluation."""
        buf = self.empty(RESULT_HEAD + extra)
        return buf, buf[:OUT_LEN], buf[OUT_LEN:OUT_LEN + 1].view(torch.int32)[:1]

    @staticmethod
    def read_result(host_buf):
        """(out, info) from a host copy of a ``result_buffer``; out as plain floats (indexing the tensor costs ~1.5 us per element)."""
        return host_buf[:OUT_LEN].tolist(), int(host_buf.numpy()[OUT_LEN:OUT_LEN + 1].view("int32")[0])

    def kuu_factor(self, Kuu, info: Optional[torch.Tensor] = None, trace_out: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, stream=None):
        """Padded L^-1 of chol(Kuu) and its info flag; independent of the streamed statistics (side-stream work).
        ``trace_out`` (``sgp_kuu_inverse_trace_len()`` doubles): also tr(K_uu^-1) in trace_out[0], from the call's own last launch
        (include/sgp.h: sgp_kuu_factor_ex; the same bits as ``kuu_inverse_trace``).  ``out`` (``sgp_kuu_factor_len(M)`` doubles) /
        ``stream``: a buffer and a stream of the caller's, as for ``kuu``."""
        M = Kuu.shape[0]
        Linv = out if out is not None else self.empty(self.lib.sgp_kuu_factor_len(M))
        if info is None:
            info = torch.empty(1, dtype=torch.int32, device=self.device)  # cleared by the call itself
        ws = self._workspace("kuu_factor", self.lib.sgp_kuu_factor_workspace_bytes(M))
        st = self.lib.sgp_ctx_kuu_factor_ex(self._c(), self._ptr(Kuu), M, self._ptr(Linv), self._ptr(info), self._ptr(trace_out), self._ptr(ws),
                                            ws.numel(), self._stream(stream))
        _lib.check("sgp_kuu_factor_ex", st)
        return Linv, info

    def kuu_inverse_trace(self, Linv, M: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tr(K_uu^-1) = ||L^-1||_F^2 in out[0] (the other entries are scratch) from ``kuu_factor``'s output: the ingredient of the
        streaming-order guard (include/sgp.h: sgp_streaming_error_estimate) that does not depend on the streamed statistics."""
        if out is None:
            out = self.empty(self.lib.sgp_kuu_inverse_trace_len())
        _lib.check("sgp_kuu_inverse_trace", self.lib.sgp_kuu_inverse_trace(self._ptr(Linv), int(M), self._ptr(out), self._stream()))
        return out

    def streaming_error_estimate(self, packed, trace, s2, N, M, result) -> None:
        """Writes the first-order estimate of |dF| / N of the streaming order into the pad word of ``result`` (a
        ``result_buffer``): it comes back with the evaluation's one host copy (``read_estimate``)."""
        buf = result[0]
        est = C.c_void_p(buf.data_ptr() + 8 * (OUT_LEN + 1))
        _lib.check("sgp_streaming_error_estimate",
                   self.lib.sgp_streaming_error_estimate(self._ptr(packed), self._ptr(trace), float(s2), int(N), int(M), est, self._stream()))

    def streaming_error_bound(self, trace, sf2, s2, result) -> None:
        """The estimate's upper bound (max Phi_ii <= N sf2^2) into the pad word of ``result``: what a whitened-order evaluation can
        still report (include/sgp.h: sgp_streaming_error_bound)."""
        est = C.c_void_p(result[0].data_ptr() + 8 * (OUT_LEN + 1))
        _lib.check("sgp_streaming_error_bound", self.lib.sgp_streaming_error_bound(self._ptr(trace), float(sf2), float(s2), est, self._stream()))

    def streaming_error_report(self, diag, stride, trace, sf2, s2, N, M, result) -> None:
        """Estimate AND upper bound into the two words behind the status word of ``result`` (include/sgp.h:
        sgp_streaming_error_report).  ``diag``: the (all-reduced) packed statistics of the streaming order with ``stride`` M + 1, the
        (all-reduced) ``phi_diag`` of the extended order with ``stride`` 1, or None (whitened order: the estimate IS the bound)."""
        est = C.c_void_p(result[0].data_ptr() + 8 * (OUT_LEN + 1))
        _lib.check("sgp_streaming_error_report",
                   self.lib.sgp_streaming_error_report(self._ptr(diag), int(stride), self._ptr(trace),
                                                       float(sf2), float(s2), int(N), int(M), est, self._stream()))

    @staticmethod
    def read_estimate(host_buf) -> float:
        return float(host_buf[OUT_LEN + 1])

    @staticmethod
    def read_bound(host_buf) -> float:
        return float(host_buf[OUT_LEN + 2])

    def bound(self, Kuu, packed, s2, N, with_adjoints=False, want_factors=False, kuu_linv=None, kuu_info=None, result=None,
              whitened=False, want_cw=False):
        """Runs the O(M^3) tail on (already all-reduced) packed statistics.

        Returns dict(out=[8] device tensor, info=int32 device tensor, buf=the ``result_buffer`` both live in, and
        when asked Phibar, bbar, Kuubar, factors; ``want_cw`` (whitened order, with adjoints) adds Cw, the whitened core
        of the adjoint that ``suffstats_bwd_factored`` takes).  Nothing is synchronised.  With ``kuu_linv`` (from ``kuu_factor``)
        the status word must already hold that call's status: pass ``result`` whose info word ``kuu_factor`` wrote,
        or ``kuu_info`` (copied in with one tiny launch).
        """
        M = Kuu.shape[0]
        self._chk(Kuu, "Kuu"), self._chk(packed, "packed")
        if whitened and kuu_linv is None:
            raise ValueError("bound(whitened=True) needs kuu_linv (the factor the statistics were whitened with)")
        buf, out, info = result if result is not None else self.result_buffer()
        if kuu_linv is not None:
            if kuu_info is not None:
                info.copy_(kuu_info)
            elif result is None:
                raise ValueError("bound(kuu_linv=...) needs the status of kuu_factor: kuu_info= or result=")
        res = {"out": out, "info": info, "buf": buf}
        Phibar = bbar = Kuubar = factors = None
        if with_adjoints:
            Phibar, bbar, Kuubar = self.empty(M, M), self.empty(M), self.empty(M, M)
            res.update(Phibar=Phibar, bbar=bbar, Kuubar=Kuubar)
        if want_factors:
            factors = self.empty(self.lib.sgp_bound_factors_len(M))
            res["factors"] = factors
        nbytes = self.lib.sgp_bound_workspace_bytes(M, 1 if with_adjoints else 0)
        ws = self._workspace("bound", nbytes)
        base = packed.data_ptr()
        stats = (C.c_void_p(base), C.c_void_p(base + 8 * M * M), C.c_void_p(base + 8 * (M * M + M)),
                 C.c_void_p(base + 8 * (M * M + M + 1)))
        tail = (float(s2), int(N), M, 1 if with_adjoints else 0, self._ptr(out), self._ptr(Phibar), self._ptr(bbar),
                self._ptr(Kuubar), self._ptr(factors), self._ptr(kuu_linv), self._ptr(info), self._ptr(ws), ws.numel(), self._stream())
        if whitened:  # (Cw = NULL: the plain whitened bound)
            if want_cw and with_adjoints:
                res["Cw"] = self.empty(M, M)
            _lib.check("sgp_bound_from_whitened_stats",
                       self.lib.sgp_ctx_bound_from_whitened_stats(self._c(), *stats, *tail[:-3], self._ptr(res.get("Cw")), *tail[-3:]))
        else:
            _lib.check("sgp_bound_from_stats", self.lib.sgp_ctx_bound_from_stats(self._c(), self._ptr(Kuu), *stats, *tail))
        return res

    def sgpmc_tail(self, packed_whitened, v, s2, N, kuu_linv, with_adjoints=False, result=None, vbar_out=None):
        """The SGPMC tail (include/sgp.h: sgp_sgpmc_from_whitened_stats) on packed whitened statistics [W | u | yy | kappa] and the
        whitened inducing values ``v`` (M doubles on the device).

        Returns dict(out = [F | data term | prior-of-v term | s2bar | kappabar] in the head of ``buf``, info, buf, and with the adjoints
        vbar, Cw, bbar, Kuubar).  ``result``: the ``result_buffer`` whose status word ``kuu_factor`` wrote -- the tail factors nothing
        and that word is the evaluation's status.  ``vbar_out`` (M doubles, e.g. a slice of the result buffer's extras): where
        vbar is written, so that it comes back with the evaluation's one host copy.  Nothing is synchronised."""
        M = int(v.numel())
        self._chk(packed_whitened, "packed_whitened"), self._chk(v, "v")
        if packed_whitened.numel() < M * M + M + 2:
            raise ValueError("packed_whitened holds %d doubles, M * M + M + 2 = %d" % (packed_whitened.numel(), M * M + M + 2))
        buf, out, info = result if result is not None else self.result_buffer()
        res = {"out": out, "info": info, "buf": buf}
        vbar = Cw = bbar = Kuubar = None
        if with_adjoints:
            if kuu_linv is None:
                raise ValueError("sgpmc_tail(with_adjoints=True) needs kuu_linv")
            self._chk(kuu_linv, "kuu_linv")
            vbar, Cw, bbar, Kuubar = vbar_out if vbar_out is not None else self.empty(M), self.empty(M, M), self.empty(M), self.empty(M, M)
            res.update(vbar=vbar, Cw=Cw, bbar=bbar, Kuubar=Kuubar)
        ws = self._workspace("sgpmc", self.lib.sgp_sgpmc_workspace_bytes(M))
        base = packed_whitened.data_ptr()
        st = self.lib.sgp_sgpmc_from_whitened_stats(
            C.c_void_p(base), C.c_void_p(base + 8 * M * M), C.c_void_p(base + 8 * (M * M + M)), C.c_void_p(base + 8 * (M * M + M + 1)),
            self._ptr(v), float(s2), int(N), M, 1 if with_adjoints else 0, self._ptr(out), self._ptr(vbar), self._ptr(Cw),
            self._ptr(bbar), self._ptr(Kuubar), self._ptr(kuu_linv), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_sgpmc_from_whitened_stats", st)
        return res

    def sgpmc_lik_rows(self, X, y, Z, ls, sf2, s2, v, kuu_linv, t_out, kernel="rbf", likelihood="poisson", want_adjoints=False):
        """The SGPMC row pass of a non-conjugate likelihood (include/sgp.h: sgp_sgpmc_lik_rows): the conditional moments of every
        datum from T = K'_fu L^-T, the likelihood layer, and the M-sized adjoints.  ``t_out`` (from ``kfu_buffer``) is required: it
        holds T on return, diag(dv) T with the adjoints -- what ``suffstats_bwd_factored(..., t_in=)`` takes.

        Returns dict(out = [sum ell | d sum ell / d s2 | sum dv], dmu, dv (N doubles), and with the adjoints g (M), G (M x M)).
        Nothing is synchronised."""
        N, d = X.shape
        M = Z.shape[0]
        self._chk(Z, "Z"), self._chk(kuu_linv, "kuu_linv"), self._chk(v, "v"), self._chk(t_out, "t_out")
        if N > 0:
            self._chk(X, "X"), self._chk(y, "y")
        if v.numel() != M:
            raise ValueError("v has %d entries, Z has %d rows" % (v.numel(), M))
        if t_out.numel() < self.lib.sgp_kfu_len(N, M):
            raise ValueError("t_out holds %d doubles, sgp_kfu_len(N, M) = %d" % (t_out.numel(), self.lib.sgp_kfu_len(N, M)))
        nbytes = self._cf.sgp_sgpmc_lik_rows_workspace_bytes(N, M, d)
        if nbytes == 0:
            raise ValueError("unsupported shape N=%d M=%d d=%d (the shard's K'_fu must fit one super-chunk)" % (N, M, d))
        ws = self._workspace("sgpmc_lik_rows", nbytes)
        res = {"out": self.empty(_lib.SGPMC_LIK_OUT_LEN), "dmu": self.empty(N), "dv": self.empty(N)}
        if want_adjoints:
            res.update(g=self.empty(M), G=self.empty(M, M))
        st = self._cf.sgp_sgpmc_lik_rows(
            self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), float(s2), self._ptr(v), N, M, d,
            _kernel_id(kernel), _likelihood_id(likelihood), self._ptr(kuu_linv), 1 if want_adjoints else 0, self._ptr(res["out"]),
            self._ptr(res.get("G")), self._ptr(res.get("g")), self._ptr(res["dmu"]), self._ptr(res["dv"]), self._ptr(t_out),
            self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_sgpmc_lik_rows", st)
        return res

    def sgpmc_lik_tail(self, rows, v, N, kuu_linv, with_adjoints=False, result=None, vbar_out=None):
        """The M x M tail behind ``sgpmc_lik_rows`` (include/sgp.h: sgp_sgpmc_lik_tail) on its result ``rows``.

        Returns dict(out = [F | sum ell | prior-of-v term | d sum ell / d s2 | (sum dv) / N] in the head of ``buf``, info, buf, and with
        the adjoints vbar, bbar, Kuubar).  ``result`` / ``vbar_out`` as for ``sgpmc_tail``.  Nothing is synchronised."""
        M = int(v.numel())
        self._chk(v, "v")
        buf, out, info = result if result is not None else self.result_buffer()
        res = {"out": out, "info": info, "buf": buf}
        vbar = bbar = Kuubar = None
        if with_adjoints:
            if kuu_linv is None or "G" not in rows:
                raise ValueError("sgpmc_lik_tail(with_adjoints=True) needs kuu_linv and the adjoints of sgpmc_lik_rows")
            self._chk(kuu_linv, "kuu_linv")
            vbar, bbar, Kuubar = vbar_out if vbar_out is not None else self.empty(M), self.empty(M), self.empty(M, M)
            res.update(vbar=vbar, bbar=bbar, Kuubar=Kuubar)
        ws = self._workspace("sgpmc", self.lib.sgp_sgpmc_lik_workspace_bytes(M))
        st = self.lib.sgp_sgpmc_lik_tail(
            self._ptr(rows["out"]), self._ptr(rows.get("G")), self._ptr(rows.get("g")), self._ptr(v), int(N), M,
            1 if with_adjoints else 0, self._ptr(out), self._ptr(vbar), self._ptr(bbar), self._ptr(Kuubar), self._ptr(kuu_linv),
            self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_sgpmc_lik_tail", st)
        return res

    def sgpmc_mc_rows(self, X, y, Z, ls, sf2, V, kuu_linv, t_out, kernel="rbf", eps=1e-3, want_adjoints=False, want_moments=False):
        """The SGPMC row pass of the multi-class robust-max likelihood (include/sgp.h: sgp_sgpmc_mc_rows).  ``V``: C x M on the device,
        class-major; ``y``: the labels 0 .. C-1 as doubles, or None for the conditional moments only (prediction).  ``t_out`` (from
        ``kfu_buffer``) holds T on return, with the adjoints the folded T_in = diag(dv) T - DMU V^T / (2 sf2) that
        ``suffstats_bwd_factored(..., t_in=)`` takes with y = 0 and bbar = 0.

        Returns dict(out = [sum ell | 0 | sum dv], dmu (C x N), dv (N); with the adjoints g (C x M), G (M x M); with ``want_moments`` or
        ``y = None`` mu (C x N), var (N)).  Nothing is synchronised."""
        N, d = X.shape
        M = Z.shape[0]
        self._chk(Z, "Z"), self._chk(kuu_linv, "kuu_linv"), self._chk(V, "V"), self._chk(t_out, "t_out")
        if V.dim() != 2 or V.shape[1] != M:
            raise ValueError("V must be C x M = ? x %d (got %s)" % (M, tuple(V.shape)))
        Cn = int(V.shape[0])
        if N > 0:
            self._chk(X, "X")
            if y is not None:
                self._chk(y, "y")
        if t_out.numel() < self.lib.sgp_kfu_len(N, M):
            raise ValueError("t_out holds %d doubles, sgp_kfu_len(N, M) = %d" % (t_out.numel(), self.lib.sgp_kfu_len(N, M)))
        if not 2 <= Cn <= _lib.SGP_MAX_CLASSES:
            raise ValueError("V has %d rows: the class count must be 2 .. %d" % (Cn, _lib.SGP_MAX_CLASSES))
        nbytes = self._cf.sgp_sgpmc_mc_rows_workspace_bytes(N, M, d, Cn)
        if nbytes == 0:
            raise ValueError("unsupported shape N=%d M=%d d=%d (the shard's K'_fu must fit one super-chunk)" % (N, M, d))
        ws = self._workspace("sgpmc_mc_rows", nbytes)
        res = {}
        if y is not None:
            res.update(out=self.empty(_lib.SGPMC_LIK_OUT_LEN), dmu=self.empty(Cn, N), dv=self.empty(N))
        if want_moments or y is None:
            res.update(mu=self.empty(Cn, N), var=self.empty(N))
        if want_adjoints:
            res.update(g=self.empty(Cn, M), G=self.empty(M, M))
        st = self._cf.sgp_sgpmc_mc_rows(
            self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), self._ptr(V), Cn, float(eps), N, M, d,
            _kernel_id(kernel), self._ptr(kuu_linv), 1 if want_adjoints else 0, self._ptr(res.get("out")), self._ptr(res.get("G")),
            self._ptr(res.get("g")), self._ptr(res.get("dmu")), self._ptr(res.get("dv")), self._ptr(res.get("mu")),
            self._ptr(res.get("var")), self._ptr(t_out), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_sgpmc_mc_rows", st)
        return res

    def sgpmc_mc_tail(self, rows, V, N, kuu_linv, with_adjoints=False, result=None, vbar_out=None):
        """The M x M tail behind ``sgpmc_mc_rows`` (include/sgp.h: sgp_sgpmc_mc_tail) on its result ``rows``.

        Returns dict(out = [F | sum ell | prior-of-V term | 0 | (sum dv) / N] in the head of ``buf``, info, buf, and with the adjoints
        vbar, bbar (C x M each), Kuubar).  ``result`` / ``vbar_out`` (C M doubles) as for ``sgpmc_tail``.  Nothing is synchronised."""
        Cn, M = int(V.shape[0]), int(V.shape[1])
        self._chk(V, "V")
        buf, out, info = result if result is not None else self.result_buffer()
        res = {"out": out, "info": info, "buf": buf}
        vbar = bbar = Kuubar = None
        if with_adjoints:
            if kuu_linv is None or "G" not in rows:
                raise ValueError("sgpmc_mc_tail(with_adjoints=True) needs kuu_linv and the adjoints of sgpmc_mc_rows")
            self._chk(kuu_linv, "kuu_linv")
            vbar, bbar, Kuubar = vbar_out if vbar_out is not None else self.empty(Cn, M), self.empty(Cn, M), self.empty(M, M)
            res.update(vbar=vbar, bbar=bbar, Kuubar=Kuubar)
        ws = self._workspace("sgpmc_mc", self.lib.sgp_sgpmc_mc_workspace_bytes(M, Cn))
        st = self.lib.sgp_sgpmc_mc_tail(
            self._ptr(rows["out"]), self._ptr(rows.get("G")), self._ptr(rows.get("g")), self._ptr(V), Cn, int(N), M,
            1 if with_adjoints else 0, self._ptr(out), self._ptr(vbar), self._ptr(bbar), self._ptr(Kuubar), self._ptr(kuu_linv),
            self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_sgpmc_mc_tail", st)
        return res

    def sgpmc_comp_rows(self, X, y, Z, block, white, s2, v, kuu_linv, t_out, likelihood="gaussian", mean=None, want_adjoints=False,
                        want_moments=False):
        """The SGPMC row pass for a composite kernel with a white-noise term and a mean function (include/sgp.h: sgp_sgpmc_comp_rows).
        ``block``: the kernel's parameter block (host list); ``white`` >= 0; ``mean`` (N doubles on the device, or None): m(x_n);
        ``kuu_linv`` from ``kuu_factor(kuu(Z, block, 1.0, jitter + white, "composite"))``.  ``y = None``: the conditional moments only
        (prediction).  ``t_out`` (from ``kfu_buffer``) holds T = K_fu L^-T on return, diag(dv) T with the adjoints -- what
        ``sgpmc_comp_bwd`` takes.

        Returns dict(out = [sum ell | d sum ell / d s2 | sum dv], dmu, dv (N), with the adjoints g (M), G (M x M), with ``want_moments``
        (or ``y = None``) mu, var (N)).  Nothing is synchronised."""
        N, d = X.shape
        M = Z.shape[0]
        self._chk(Z, "Z"), self._chk(kuu_linv, "kuu_linv"), self._chk(v, "v"), self._chk(t_out, "t_out")
        if N > 0:
            self._chk(X, "X")
            for t, name in ((y, "y"), (mean, "mean")):
                if t is not None and (self._chk(t, name).numel() != N):
                    raise ValueError("%s has %d entries, X has %d rows" % (name, t.numel(), N))
        if v.numel() != M:
            raise ValueError("v has %d entries, Z has %d rows" % (v.numel(), M))
        if t_out.numel() < self.lib.sgp_kfu_len(N, M):
            raise ValueError("t_out holds %d doubles, sgp_kfu_len(N, M) = %d" % (t_out.numel(), self.lib.sgp_kfu_len(N, M)))
        if y is None and want_adjoints:
            raise ValueError("sgpmc_comp_rows(y=None) returns the moments only: there are no adjoints")
        nbytes = self._cf.sgp_sgpmc_comp_rows_workspace_bytes(N, M, d)
        if nbytes == 0:
            raise ValueError("unsupported shape N=%d M=%d d=%d (a composite kernel takes d <= 8)" % (N, M, d))
        ws = self._workspace("sgpmc_comp_rows", nbytes)
        res = {"out": self.empty(_lib.SGPMC_LIK_OUT_LEN), "dmu": self.empty(N), "dv": self.empty(N)}
        if want_adjoints:
            res.update(g=self.empty(M), G=self.empty(M, M))
        if want_moments or y is None:
            res.update(mu=self.empty(N), var=self.empty(N))
        st = self._cf.sgp_sgpmc_comp_rows(
            self._ptr(X), d, self._ptr(y), self._ptr(mean), self._ptr(Z), d, self._inv_ls(block, d, "composite"), float(white), float(s2),
            self._ptr(v), N, M, d, _likelihood_id(likelihood), self._ptr(kuu_linv), 1 if want_adjoints else 0, self._ptr(res["out"]),
            self._ptr(res.get("G")), self._ptr(res.get("g")), self._ptr(res["dmu"]), self._ptr(res["dv"]), self._ptr(res.get("mu")),
            self._ptr(res.get("var")), self._ptr(t_out), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_sgpmc_comp_rows", st)
        return res

    def sgpmc_comp_bwd(self, X, dmu, Z, block, t_in, kuu_linv, bbar, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The N-side gradient behind ``sgpmc_comp_rows`` (include/sgp.h: sgp_sgpmc_comp_bwd): ``out[:COMP_LEN]`` is overwritten with
        sum_nm Kfubar_nm dk(x_n, z_m)/d block, Kfubar = -2 t_in L^-1 + dmu bbar^T (``t_in``: ``t_out`` after a call with the adjoints,
        ``bbar`` = L^-T v from ``sgpmc_lik_tail``).  ``out`` holds COMP_LEN + 1 doubles, the layout ``kuu_bwd(kernel="composite")`` adds
        the K_uu side into.  Nothing is synchronised."""
        N, d = X.shape
        M = Z.shape[0]
        self._chk(Z, "Z"), self._chk(kuu_linv, "kuu_linv"), self._chk(t_in, "t_in"), self._chk(bbar, "bbar")
        if N > 0:
            self._chk(X, "X"), self._chk(dmu, "dmu")
        if out is None:
            out = self.empty(COMP_LEN + 1)
            out[COMP_LEN:].zero_()
        nbytes = self._cf.sgp_sgpmc_comp_bwd_workspace_bytes(N, M, d)
        if nbytes == 0:
            raise ValueError("unsupported shape N=%d M=%d d=%d (a composite kernel takes d <= 8)" % (N, M, d))
        ws = self._workspace("sgpmc_comp_bwd", nbytes)
        st = self._cf.sgp_sgpmc_comp_bwd(self._ptr(X), d, self._ptr(dmu), self._ptr(Z), d, self._inv_ls(block, d, "composite"),
                                         self._ptr(t_in), self._ptr(kuu_linv), self._ptr(bbar), N, M, d, C.c_void_p(out.data_ptr()),
                                         self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_sgpmc_comp_bwd", st)
        return out

    # ------------------------------------------------------------------ single-launch path for small problems
    def small_supported(self, N: int, M: int, d: int, kernel="rbf") -> bool:
        return bool(self._cf.sgp_small_supported(int(N), int(M), int(d), _kernel_id(kernel)))

    def _small_ws(self, N, M, d, nbytes=None):
        """nbytes: at least this many (sgp_small_nuts_joint's workspace extends the single-launch one)."""
        base = self.lib.sgp_small_workspace_bytes(N, M, d)
        if base == 0:
            raise ValueError("shape N=%d M=%d d=%d is outside the single-launch path" % (N, M, d))
        nbytes = max(int(nbytes or 0), int(base))
        # one workspace per HIP stream: the launch's sync words live in it, so two evaluations in flight on different streams
        # of one engine must not share them
        key = ("small", int(torch.cuda.current_stream(self.device).cuda_stream) if self.device.type == "cuda" else 0)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.zeros(int(nbytes), dtype=torch.uint8, device=self.device)  # zeroed once: the sync words
            self._ws[key] = ws
        return ws

    @staticmethod
    def _composite_args(composite, hmc: bool):
        """(structure, n_free, slots, roles, sds) ctypes arguments of the *_composite entry points (host arrays).
        ``composite`` = {"structure": the SGP_COMP_LEN parameter block, "free": [(slot, role 0 amp / 1 ls / 2 aux, prior sd)]}."""
        blk = [float(v) for v in composite["structure"]]
        if len(blk) != _lib.COMP_LEN:
            raise ValueError("composite structure must have %d entries" % _lib.COMP_LEN)
        free = list(composite.get("free") or []) if hmc else []
        n = len(free)
        return ((C.c_double * len(blk))(*blk), n, (C.c_int * max(n, 1))(*[int(f[0]) for f in free]),
                (C.c_int * max(n, 1))(*[int(f[1]) for f in free]), (C.c_double * max(n, 1))(*[float(f[2]) for f in free]))

    @staticmethod
    def small_out_len(d: int, mode: int = 0, composite=None) -> int:
        """Entries of the result of one evaluation: [value | kernel hyper-parameter gradients | noise | logmarg | trace]."""
        if composite is None:
            return d + 5
        return (len(composite["free"]) if mode else _lib.COMP_LEN) + 4

    def small_eval(self, X, y, Z, theta: torch.Tensor, jitter, kernel="rbf", mode=0, want_grad=True, want_gz=False,
                   out: Optional[torch.Tensor] = None, composite=None):
        """ONE kernel launch: the bound (mode 0) or the NUTS target (mode 1) and its gradient, hyper-parameters read from
        the device tensor ``theta``.  Returns (out device tensor, gZ or None, info int32 device tensor); nothing is
        synchronised.  ``out`` may be a caller-owned buffer of ``small_out_len`` (+1 for the status word, see
        ``small_result``) entries.  ``kernel="composite"``: ``composite`` carries the structure (see ``_composite_args``);
        theta = [parameter block | s2] (mode 0) or [log free parameters | log sigma] (mode 1); no dF/dZ."""
        N, d = X.shape
        M = Z.shape[0]
        for t, n in ((X, "X"), (y, "y"), (Z, "Z"), (theta, "theta")):
            self._chk(t, n)
        is_comp = _kernel_id(kernel) == _kernel_id("composite")
        if is_comp != (composite is not None):
            raise ValueError("composite= goes with kernel='composite'")
        nout = self.small_out_len(d, mode, composite)
        if theta.numel() != nout - 3:
            raise ValueError("theta has %d entries, expected %d" % (theta.numel(), nout - 3))
        ws = self._small_ws(N, M, d)
        if out is None:
            out, info = self.small_result(nout - 5)
        else:
            info = out[nout:nout + 1].view(torch.int32)[:1]
        if is_comp:
            if want_gz:
                raise ValueError("the single-launch path has no dF/dZ for composite kernels")
            cargs = self._composite_args(composite, bool(mode))
            st = self._cf.sgp_small_eval_composite(self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._ptr(theta), *cargs, N, M, d,
                                                   float(jitter), int(mode), 1 if want_grad else 0, self._ptr(out),
                                                   C.c_void_p(info.data_ptr()), self._ptr(ws), ws.numel(), self._stream())
            _lib.check("sgp_small_eval_composite", st)
            return out, None, info
        gz = self.empty(M, d) if (want_grad and want_gz) else None
        st = self._cf.sgp_small_eval(self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._ptr(theta), N, M, d, _kernel_id(kernel),
                                     float(jitter), int(mode), 1 if want_grad else 0, self._ptr(out), self._ptr(gz),
                                     C.c_void_p(info.data_ptr()), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_small_eval", st)
        return out, gz, info

    def small_eval_batch(self, X, y, Z, thetas: torch.Tensor, jitter, kernel="rbf", mode=0, want_grad=True, want_gz=False):
        """S evaluations (``thetas``: S x (d + 2) on the device) in one launch.  Returns (outs [S, d + 5], gZ [S, M, d] or None,
        infos [S] int32), device tensors; nothing is synchronised."""
        N, d = X.shape
        M = Z.shape[0]
        for t, n in ((X, "X"), (y, "y"), (Z, "Z"), (thetas, "thetas")):
            self._chk(t, n)
        S = thetas.shape[0]
        if thetas.shape[1] != d + 2:
            raise ValueError("thetas must be S x (d + 2)")
        ws = self._small_ws(N, M, d)
        outs = self.empty(S, d + 5)
        gz = self.empty(S, M, d) if (want_grad and want_gz) else None
        infos = torch.zeros(S, dtype=torch.int32, device=self.device)
        scratch = self.empty(d + 2)
        st = self._cf.sgp_small_eval_batch(self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._ptr(thetas), S, N, M, d,
                                           _kernel_id(kernel), float(jitter), int(mode), 1 if want_grad else 0, self._ptr(scratch),
                                           self._ptr(outs), self._ptr(gz), C.c_void_p(infos.data_ptr()), self._ptr(ws), ws.numel(),
                                           self._stream())
        _lib.check("sgp_small_eval_batch", st)
        return outs, gz, infos

    def _nuts_buffers(self, n_draws, nd, n_counters):
        """(samples, stats, counters, info) device buffers of one persistent sampler launch."""
        cols = int(self.lib.sgp_small_nuts_stat_cols())
        return (self.empty(n_draws, nd), torch.zeros(n_draws * cols, dtype=torch.float64, device=self.device),
                torch.zeros(n_counters, dtype=torch.int64, device=self.device), torch.zeros(1, dtype=torch.int32, device=self.device))

    def _nuts_result(self, samples, stats, counters, info):
        """The launch's buffers as host tensors / ints (synchronises); counters 2 and 3, where the launch has them, are the
        joint sampler's device times in units of 1e-8 s."""
        n_draws, cols = samples.shape[0], int(self.lib.sgp_small_nuts_stat_cols())
        h = stats.to("cpu")
        c = counters.to("cpu")
        res = {"samples": samples.to("cpu"), "stats": h[: n_draws * (cols - 1)].reshape(n_draws, cols - 1),
               "seconds": h[n_draws * (cols - 1):], "evaluations": int(c[0]), "draws": int(c[1]), "info": int(info.to("cpu")[0])}
        if c.numel() == 4:
            res.update(sampler_seconds=int(c[2]) * 1e-8, eval_seconds=int(c[3]) * 1e-8)
        if res["info"] < 0:
            self.small_reset()
        return res

    def small_nuts(self, X, y, Z, q0, n_tune, n_draws, seed, jitter=1e-6, kernel="rbf", max_treedepth=10, step_scale=0.25,
                   target_accept=0.8, composite=None):
        """The whole NUTS run in one persistent launch (sgp_small_nuts / sgp_small_nuts_composite).  Returns dict(samples
        [n_draws, ndim] unconstrained, stats [n_draws, 8], seconds [n_draws], evaluations, draws, info) as host tensors /
        ints (synchronises).  ndim = d + 2, or the composite kernel's free parameters + 1."""
        N, d = X.shape
        M = Z.shape[0]
        for t, n in ((X, "X"), (y, "y"), (Z, "Z")):
            self._chk(t, n)
        is_comp = _kernel_id(kernel) == _kernel_id("composite")
        if is_comp != (composite is not None):
            raise ValueError("composite= goes with kernel='composite'")
        nout = self.small_out_len(d, 1, composite)
        nd = nout - 3
        q0d = torch.as_tensor([float(v) for v in q0], dtype=torch.float64).to(self.device)
        if q0d.numel() != nd:
            raise ValueError("q0 has %d entries, expected %d" % (q0d.numel(), nd))
        ws = self._small_ws(N, M, d)
        samples, stats, counters, info = self._nuts_buffers(n_draws, nd, 2)
        theta, out = self.empty(nd), self.empty(nout)
        head = (self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._ptr(q0d))
        tail = (float(jitter), int(n_tune), int(n_draws), int(max_treedepth), float(step_scale), float(target_accept),
                int(seed) & ((1 << 64) - 1), self._ptr(theta), self._ptr(samples), self._ptr(stats),
                C.c_void_p(counters.data_ptr()), self._ptr(out), C.c_void_p(info.data_ptr()), self._ptr(ws), ws.numel(),
                self._stream())
        if is_comp:
            cargs = self._composite_args(composite, True)
            _lib.check("sgp_small_nuts_composite", self._cf.sgp_small_nuts_composite(*head, *cargs, N, M, d, *tail))
        else:
            _lib.check("sgp_small_nuts", self._cf.sgp_small_nuts(*head, N, M, d, _kernel_id(kernel), *tail))
        return self._nuts_result(samples, stats, counters, info)

    def small_nuts_joint(self, X, y, M, q0, n_tune, n_draws, seed, jitter=1e-6, kernel="rbf", max_treedepth=10, step_scale=0.25,
                         target_accept=0.8):
        """Joint NUTS over theta and the M x d inducing inputs in one persistent launch (sgp_small_nuts_joint); q0 = [log ls,
        log sig_f, log sig_n, vec(Z)].  Returns the dict of ``small_nuts`` (samples [n_draws, d + 2 + M d]) plus the device
        seconds workgroup 0 spent in the sampler and in the evaluations (``sampler_seconds``, ``eval_seconds``)."""
        N, d = X.shape
        M = int(M)
        for t, n in ((X, "X"), (y, "y")):
            self._chk(t, n)
        if _kernel_id(kernel) == _kernel_id("composite"):
            raise ValueError("the joint sampler takes stationary kernels")
        nd = d + 2 + M * d
        q0d = torch.as_tensor(np.asarray(q0, dtype=np.float64).reshape(-1)).to(self.device)
        if q0d.numel() != nd:
            raise ValueError("q0 has %d entries, expected %d" % (q0d.numel(), nd))
        nbytes = self.lib.sgp_small_nuts_joint_workspace_bytes(N, M, d)
        if nbytes == 0:
            raise ValueError("shape N=%d M=%d d=%d is outside the single-launch path" % (N, M, d))
        small = self._small_ws(N, M, d, nbytes)  # the per-stream single-launch workspace, sized to hold the sampler's vectors too
        samples, stats, counters, info = self._nuts_buffers(n_draws, nd, 4)
        out = self.empty(d + 5)
        _lib.check("sgp_small_nuts_joint", self._cf.sgp_small_nuts_joint(
            self._ptr(X), d, self._ptr(y), self._ptr(q0d), N, M, d, _kernel_id(kernel), float(jitter), int(n_tune), int(n_draws),
            int(max_treedepth), float(step_scale), float(target_accept), int(seed) & ((1 << 64) - 1), self._ptr(samples),
            self._ptr(stats), C.c_void_p(counters.data_ptr()), self._ptr(out), C.c_void_p(info.data_ptr()), self._ptr(small),
            small.numel(), self._stream()))
        return self._nuts_result(samples, stats, counters, info)

    def small_result(self, d: int):
        """[out (d + 5) | status word] in one buffer, so one device-to-host copy ends an evaluation."""
        buf = self.empty(d + 6)
        return buf, buf[d + 5:d + 6].view(torch.int32)[:1]

    def small_reset(self):
        """Zero the sync words again (only needed after a SGP_INFO_TIMEOUT)."""
        for key, ws in self._ws.items():
            if isinstance(key, tuple) and key[0] == "small":
                ws[: self.lib.sgp_small_sync_bytes()].zero_()

    # ------------------------------------------------------------------ pass 2
    def suffstats_bwd(self, X, y, Z, ls, sf2, Phibar, bbar, kappabar, kernel="rbf", want_gz=False,
                      out: Optional[torch.Tensor] = None, kfu: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Packed local gradients [g_hyper (d lengthscales, or the composite block) | g_sf2 | g_Z (M*d, only when want_gz)]."""
        N, d = X.shape
        M = Z.shape[0]
        nh = self.hyper_len(kernel, d)
        if out is None:
            out = self.empty(nh + 1 + (M * d if want_gz else 0))
        nbytes = self.lib.sgp_suffstats_bwd_workspace_bytes_ex(N, M, d, 1 if kfu is not None else 0)
        ws = self._workspace("bwd_kfu" if kfu is not None else "bwd", nbytes)
        base = out.data_ptr()
        st = self.lib.sgp_ctx_suffstats_bwd(
            self._c(), self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), self._ptr(Phibar),
            self._ptr(bbar), float(kappabar), self._ptr(kfu), N, M, d, _kernel_id(kernel), C.c_void_p(base),
            C.c_void_p(base + 8 * nh),
            C.c_void_p(base + 8 * (nh + 1)) if want_gz else C.c_void_p(0), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_suffstats_bwd", st)
        return out

    def suffstats_bwd_factored(self, X, y, Z, ls, sf2, kuu_linv, Cw, s2, bbar, kappabar, kernel="rbf", want_gz=False,
                               out: Optional[torch.Tensor] = None, t_in: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``suffstats_bwd`` from the factored adjoint 2 s2 Phibar = L^-T Cw L^-1 (``kuu_linv`` from ``kuu_factor``, ``Cw``
        from ``bound(..., whitened=True, want_cw=True)``): same packed gradients, without the cancellation of an explicit
        Phibar on ill-conditioned K_uu.  ``t_in``: T = K'_fu L^-T kept by ``suffstats_whitened_rows(..., t_out=)``."""
        N, d = X.shape
        M = Z.shape[0]
        nh = self.hyper_len(kernel, d)
        if out is None:
            out = self.empty(nh + 1 + (M * d if want_gz else 0))
        if t_in is not None:
            self._chk(t_in, "t_in")
        nbytes = self.lib.sgp_ctx_suffstats_bwd_factored_workspace_bytes(self._c(), N, M, d, 1 if t_in is not None else 0)
        ws = self._workspace("bwd_factored_t" if t_in is not None else "bwd_factored", nbytes)
        base = out.data_ptr()
        st = self.lib.sgp_ctx_suffstats_bwd_factored(
            self._c(), self._ptr(X), d, self._ptr(y), self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), self._ptr(kuu_linv),
            self._ptr(Cw), float(s2), self._ptr(bbar), float(kappabar), N, M, d, _kernel_id(kernel),
            self._ptr(t_in), C.c_void_p(base),
            C.c_void_p(base + 8 * nh), C.c_void_p(base + 8 * (nh + 1)) if want_gz else C.c_void_p(0), self._ptr(ws), ws.numel(),
            self._stream())
        _lib.check("sgp_suffstats_bwd_factored_ex", st)
        return out

    def kuu_bwd(self, Z, ls, sf2, Kuubar, grads: torch.Tensor, kernel="rbf", want_gz=False) -> torch.Tensor:
        """Adds the Kuu path into the packed gradient buffer produced by ``suffstats_bwd``."""
        M, d = Z.shape
        nbytes = self.lib.sgp_kuu_bwd_workspace_bytes(M, d)
        ws = self._workspace("kuu_bwd", nbytes)
        base = grads.data_ptr()
        nh = self.hyper_len(kernel, d)
        st = self.lib.sgp_kuu_bwd(
            self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), self._ptr(Kuubar), M, d, _kernel_id(kernel),
            C.c_void_p(base), C.c_void_p(base + 8 * nh), C.c_void_p(base + 8 * (nh + 1)) if want_gz else C.c_void_p(0),
            self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_kuu_bwd", st)
        return grads

    # ------------------------------------------------------------------ predictive
    def predict(self, Xs, Z, ls, sf2, s2, factors, kernel="rbf", pred_noise=True, full_cov=False):
        T, d = Xs.shape
        M = Z.shape[0]
        self._chk(Xs, "Xs"), self._chk(factors, "factors")
        mean, var = self.empty(T), self.empty(T)
        cov = self.empty(T, T) if full_cov else None
        nbytes = self.lib.sgp_predict_workspace_bytes(T, M, d, 1 if full_cov else 0)
        ws = self._workspace("predict", nbytes)
        st = self._cf.sgp_predict(
            self._ptr(Xs), d, T, self._ptr(Z), d, self._inv_ls(ls, d, kernel), float(sf2), float(s2), self._ptr(factors), M, d,
            _kernel_id(kernel), 1 if pred_noise else 0, self._ptr(mean), self._ptr(var), self._ptr(cov),
            self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_predict", st)
        return mean, var, cov

    # ------------------------------------------------------------------ exact GP marginal likelihood (GPR_HMC)
    EXACT_HEAD = 6  # doubles ahead of the gradient in an exact_eval result buffer: out (4) | status word | pad

    def exact_eval(self, X, y, ls, sf2, s2, kernel="rbf", want_grad=True, want_factors=False):
        """log N(y | 0, K(X, X) + s2 I) and, with ``want_grad``, its gradient (include/sgp.h: sgp_exact_eval).  Everything the host
        reads -- F, y^T A^-1 y, log|A|, tr A^-1, the status word and the d + 2 gradient entries -- lands in ONE result buffer that
        comes back in one device-to-host copy.  Returns dict(F, out=[4 floats], info, and with ``want_grad`` ls=[d], sf2, s2; with
        ``want_factors`` factors= the opaque device buffer ``exact_predict`` consumes).  A non-zero ``info`` (A numerically not
        positive definite, the conditioning gate, a time-out) is reported, never raised."""
        N, d = X.shape
        self._chk(X, "X"), self._chk(y, "y")
        H = self.EXACT_HEAD
        buf = self.empty(H + d + 2)
        info = buf[4:5].view(torch.int32)[:1]
        factors = self.empty(self.lib.sgp_exact_factors_len(N)) if want_factors else None
        ws = self._workspace("exact", self.lib.sgp_exact_workspace_bytes(N, d, 1 if want_grad else 0))
        base = buf.data_ptr()
        st = self.lib.sgp_ctx_exact_eval(
            self._c(), self._ptr(X), d, self._ptr(y), N, d, self._inv_ls(ls, d, kernel), float(sf2), float(s2), _kernel_id(kernel),
            1 if want_grad else 0, C.c_void_p(base), C.c_void_p(base + 8 * H) if want_grad else C.c_void_p(0), self._ptr(factors),
            self._ptr(info), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_exact_eval", st)
        host = buf.to("cpu")
        vals = host.tolist()
        res = {"F": vals[0], "out": vals[:4], "info": int(host[4:5].numpy().view("int32")[0])}
        if want_grad:
            res.update(ls=vals[H:H + d], sf2=vals[H + d], s2=vals[H + d + 1])
        if want_factors:
            res["factors"] = factors
        return res

    # ------------------------------------------------------------------ the one-workgroup-per-problem libraries: their shared frame
    def _companion_lib(key, what):  # noqa: N805 - builds the properties below
        return property(lambda self: _lib._load_companion(key), doc="The companion library of %s, loaded on first use." % what)

    exact_nuts_lib = _companion_lib("exact_nuts", "the batched sampler (include/sgp_exact_nuts.h)")
    exact_predict_lib = _companion_lib("exact_predict", "the batched predictive (include/sgp_exact_predict.h)")
    vfe_batch_lib = _companion_lib("vfe_batch", "the batched collapsed bound (include/sgp_vfe_batch.h)")
    vfe_nuts_lib = _companion_lib("vfe_nuts", "the batched sparse sampler (include/sgp_vfe_nuts.h)")
    vfe_predict_lib = _companion_lib("vfe_predict", "the batched sparse predictive (include/sgp_vfe_predict.h)")
    mixture_lib = _companion_lib("mixture", "the mixture quantiles (include/sgp_mixture.h)")
    del _companion_lib

    @staticmethod
    def _set_index(device, idx, name: str, n_sets: int, P: int):
        """A set index (ix / iy / iz / ixs) as a device int32 tensor of P entries, or None.  A host sequence is range-checked here (it
        costs nothing); a device tensor is taken as it is -- the caller answers for its range, nothing is copied to the host."""
        if idx is None:
            return None
        if isinstance(idx, torch.Tensor) and idx.device == device:
            if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.numel() != P:
                raise ValueError("%s must be a contiguous int32 tensor of %d entries" % (name, P))
            return idx
        host = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx).reshape(-1)
        if host.size != P or (P and (host.min() < 0 or host.max() >= n_sets)):
            raise ValueError("%s must hold %d indices in [0, %d)" % (name, P, n_sets))
        return torch.as_tensor(host.astype(np.int32), device=device)

    @staticmethod
    def _batch_intake(device, X, Y, Z=None, theta=None, Xs=None, idx=(), limits=None, own=None):
        """The intake of every batched entry point, by the names of its tensors: X (sets x N x d), Y (sets x N) and, where the caller
        has them, Z (sets x M x d), Xs (sets x T x d) -- a tensor one rank short is lifted to one set -- and theta (P x (d + 2), taken
        as it is).  Every tensor must be contiguous float64 on ``device``.  A sampler has no theta and passes ``own`` = (its P, whether
        its own arguments fit, the tail of the refusal) instead.  What does not fit is refused with "shapes: X ..., Y ..., ..." over
        exactly the tensors passed (theta last).  Then the VFE family's ``limits`` = (entry point, "P" or "C") where given
        (``_vfe_limits``), and the set indices ``idx`` -- ix, iy[, iz][, ixs]: one per tensor passed but theta -- through
        ``_set_index``.  Returns ((X, Y, Z, Xs) as lifted, the indices, (N, d, M, T, P)); None for what was not passed.  It runs on
        CPU tensors as well."""
        X = X if X.dim() == 3 else X[None]
        Y = Y if Y.dim() == 2 else Y[None]
        nX, N, d = X.shape
        _chk(device, X, "X"), _chk(device, Y, "Y")
        shape = Y.shape
        sets, ok, M, T = [("ix", nX), ("iy", shape[0])], shape[1] == N, None, None
        if Z is not None:
            Z = _chk(device, Z if Z.dim() == 3 else Z[None], "Z")
            shape = Z.shape
            sets.append(("iz", shape[0]))
            M, ok = shape[1], ok and shape[2] == d
        if theta is not None:
            _chk(device, theta, "theta")
        if Xs is not None:
            Xs = _chk(device, Xs if Xs.dim() == 3 else Xs[None], "Xs")
            shape = Xs.shape
            sets.append(("ixs", shape[0]))
            T, ok = shape[1], ok and shape[2] == d
        if theta is None:
            P, fits, tail = own
            ok = ok and fits
        elif ok and theta.dim() == 2 and theta.shape[1] == d + 2:
            P = theta.shape[0]
        else:
            ok, tail = False, ", theta %s (expected theta P x %d)" % (tuple(theta.shape), d + 2)
        if not ok:
            passed = [(n, t) for n, t in (("X", X), ("Y", Y), ("Z", Z), ("Xs", Xs)) if t is not None]
            raise ValueError("shapes: " + ", ".join("%s %s" % (n, tuple(t.shape)) for n, t in passed) + tail)
        if limits is not None:
            HipEngine._vfe_limits(limits[0], limits[1], M, N, d, P, T)
        return (X, Y, Z, Xs), [HipEngine._set_index(device, i, *s, P) for i, s in zip(idx, sets)], (N, d, M, T, P)

    @staticmethod
    def _vfe_limits(fn: str, count: str, M, N, d, P, T=None):
        """The limits of the collapsed-bound family (``_lib.VFE_BATCH_MAX_*``, and VFE_PREDICT_MAX_T where there is a T), refused in
        the words of the entry point ``fn`` that counts its problems as ``count`` ("P" or "C")."""
        if not (1 <= M <= _lib.VFE_BATCH_MAX_M and 1 <= N <= _lib.VFE_BATCH_MAX_N and 1 <= d <= _lib.VFE_BATCH_MAX_D
                and 1 <= P <= _lib.VFE_BATCH_MAX_P and (T is None or 1 <= T <= _lib.VFE_PREDICT_MAX_T)):
            lim, got = (", 1 <= T <= %d and" % _lib.VFE_PREDICT_MAX_T, ", T %d" % T) if T is not None else (" and", "")
            raise ValueError("%s takes 1 <= M <= %d, 1 <= N <= %d, 1 <= d <= %d%s 1 <= %s < 2^24 (got M %d, N %d, d %d%s, %s %d)"
                             % (fn, _lib.VFE_BATCH_MAX_M, _lib.VFE_BATCH_MAX_N, _lib.VFE_BATCH_MAX_D, lim, count, M, N, d, got, count, P))

    def exact_eval_batch(self, X, Y, theta, ix=None, iy=None, kernel="rbf", want_grad=True):
        """P exact marginal likelihoods in ONE launch (include/sgp.h: sgp_exact_eval_batch).  X: nX x N x d (or N x d), Y: nY x N (or
        N), theta: P x (d + 2) rows [ls_1..d | sf2 | s2] -- device tensors; problem p takes data set ix[p] and target iy[p] (None: set
        0).  Returns device tensors (F [P], out [P, 4], grads [P, d + 2] or None, info [P] int32); nothing is synchronised and nothing
        is copied to the host.  A problem with info != 0 has NaN rows."""
        (X, Y, _, _), (ix, iy), (N, d, _, _, P) = self._batch_intake(self.device, X, Y, theta=theta, idx=(ix, iy))
        out = self.empty(P, 4)
        grads = self.empty(P, d + 2) if want_grad else None
        info = torch.empty(P, dtype=torch.int32, device=self.device)
        ws = self._workspace("exact_batch", self.lib.sgp_exact_batch_workspace_bytes(P, N, d, 1 if want_grad else 0))
        st = self.lib.sgp_ctx_exact_eval_batch(
            self._c(), self._ptr(X), N * d, d, self._ptr(Y), N, self._ptr(ix), self._ptr(iy), self._ptr(theta), P, N, d,
            _kernel_id(kernel), 1 if want_grad else 0, self._ptr(out), self._ptr(grads), self._ptr(info), self._ptr(ws), ws.numel(),
            self._stream())
        _lib.check("sgp_exact_eval_batch", st)
        return out[:, 0], out, grads, info

    def vfe_eval_batch(self, X, Y, Z, theta, ix=None, iy=None, iz=None, kernel="rbf", jitter=1e-6, want_grad=True, want_gz=False):
        """P collapsed (VFE) bounds with their gradients in ONE launch, one workgroup per problem (include/sgp_vfe_batch.h:
        sgp_vfe_eval_batch).  X: nX x N x d (or N x d), Y: nY x N (or N), Z: nZ x M x d (or M x d), theta: P x (d + 2) rows [ls_1..d |
        sf2 | s2] -- device tensors; problem p takes data set ix[p], target iy[p] and inducing set iz[p] (None: set 0).  Returns device
        tensors (out [P, d + 5] = [F | dF/dls | dF/dsf2 | dF/ds2 | logmarg | trace], g_Z [P, M, d] or None, info [P] int32); nothing is
        synchronised and nothing is copied to the host.  A problem with info != 0 has NaN rows."""
        (X, Y, Z, _), (ix, iy, iz), (N, d, M, _, P) = self._batch_intake(self.device, X, Y, Z, theta, None, (ix, iy, iz), ("vfe_eval_batch", "P"))
        out = self.empty(P, d + 5)
        gz = self.empty(P, M, d) if want_grad and want_gz else None
        info = torch.empty(P, dtype=torch.int32, device=self.device)
        lib = self.vfe_batch_lib
        ws = self._workspace("vfe_batch", lib.sgp_vfe_batch_workspace_bytes(P, N, M, d, 1 if want_grad else 0, 1 if gz is not None else 0))
        st = lib.sgp_ctx_vfe_eval_batch(
            self._c(), self._ptr(X), N * d, d, self._ptr(Y), N, self._ptr(ix), self._ptr(iy), self._ptr(Z), M * d, d, self._ptr(iz),
            self._ptr(theta), P, N, M, d, _kernel_id(kernel), float(jitter), 1 if want_grad else 0, self._ptr(out), self._ptr(gz),
            self._ptr(info), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_vfe_eval_batch", st)
        return out, gz, info

    def vfe_predict_batch(self, X, Y, Z, theta, Xs, ix=None, iy=None, iz=None, ixs=None, kernel="rbf", jitter=1e-6, pred_noise=True,
                          want_bound=True):
        """The predictive of P collapsed (VFE) sparse GPs in ONE launch, one workgroup per problem (include/sgp_vfe_predict.h:
        sgp_vfe_predict_batch).  X: nX x N x d (or N x d), Y: nY x N (or N), Z: nZ x M x d (or M x d), Xs: nT x T x d (or T x d), theta:
        P x (d + 2) rows [ls_1..d | sf2 | s2] -- device tensors; problem p takes data set ix[p], target iy[p], inducing set iz[p] and
        test set ixs[p] (None: set 0); ``jitter`` goes on K_uu.  Returns device tensors (mean [P, T], var [P, T], bound [P] -- the
        collapsed bound F of every problem, with the bits ``vfe_eval_batch(want_grad=False)`` gives; None without ``want_bound`` --,
        info [P] int32); nothing is synchronised and nothing is copied to the host.  A problem with info != 0 has NaN rows."""
        (X, Y, Z, Xs), (ix, iy, iz, ixs), (N, d, M, T, P) = self._batch_intake(
            self.device, X, Y, Z, theta, Xs, (ix, iy, iz, ixs), ("vfe_predict_batch", "P"))
        mean, var = self.empty(P, T), self.empty(P, T)
        bound = self.empty(P) if want_bound else None
        info = torch.empty(P, dtype=torch.int32, device=self.device)
        lib = self.vfe_predict_lib
        ws = self._workspace("vfe_predict", lib.sgp_vfe_predict_batch_workspace_bytes(P, N, M, d, T))
        st = lib.sgp_ctx_vfe_predict_batch(
            self._c(), self._ptr(X), N * d, d, self._ptr(Y), N, self._ptr(ix), self._ptr(iy), self._ptr(Z), M * d, d, self._ptr(iz),
            self._ptr(Xs), T * d, d, T, self._ptr(ixs), self._ptr(theta), P, N, M, d, _kernel_id(kernel), float(jitter),
            1 if pred_noise else 0, self._ptr(mean), self._ptr(var), self._ptr(bound), self._ptr(info), self._ptr(ws), ws.numel(),
            self._stream())
        _lib.check("sgp_vfe_predict_batch", st)
        return mean, var, bound, info

    def exact_predict_batch(self, X, Y, theta, Xs, ix=None, iy=None, ixs=None, kernel="rbf", pred_noise=True):
        """The exact-GP predictive of P problems in ONE launch (include/sgp_exact_predict.h: sgp_exact_predict_batch).  X: nX x N x d (or
        N x d), Y: nY x N (or N), Xs: nT x T x d (or T x d), theta: P x (d + 2) rows [ls_1..d | sf2 | s2] -- device tensors; problem p
        takes data set ix[p], target iy[p] and test set ixs[p] (None: set 0).  Returns device tensors (mean [P, T], var [P, T], info
        [P] int32); nothing is synchronised and nothing is copied to the host.  A problem with info != 0 has NaN rows."""
        (X, Y, _, Xs), (ix, iy, ixs), (N, d, _, T, P) = self._batch_intake(self.device, X, Y, theta=theta, Xs=Xs, idx=(ix, iy, ixs))
        mean, var = self.empty(P, T), self.empty(P, T)
        info = torch.empty(P, dtype=torch.int32, device=self.device)
        lib = self.exact_predict_lib
        ws = self._workspace("exact_predict_batch", lib.sgp_exact_predict_batch_workspace_bytes(P, N, d, T))
        st = lib.sgp_ctx_exact_predict_batch(
            self._c(), self._ptr(X), N * d, d, self._ptr(Y), N, self._ptr(Xs), T * d, d, T, self._ptr(ix), self._ptr(iy), self._ptr(ixs),
            self._ptr(theta), P, N, d, _kernel_id(kernel), 1 if pred_noise else 0, self._ptr(mean), self._ptr(var), self._ptr(info),
            self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_exact_predict_batch", st)
        return mean, var, info

    def exact_mixture(self, mean, var, info, offsets, Ytest=None):
        """The mixture over the draws of each group in ONE launch (sgp_exact_mixture_reduce): rows [offsets[g], offsets[g + 1]) of mean /
        var (P x T, device) are the draws of group g; ``offsets`` is a host sequence, non-decreasing from 0 to P.  Draws with info != 0
        are left out.  Returns a dict of device tensors: mean, var [G, T], kept [G] int32, and with ``Ytest`` (G x T) logpdf (the log
        of the mean density) and mean_logpdf [G, T] (None without).  A group with no draw left is NaN.  Nothing is synchronised."""
        self._chk(mean, "mean"), self._chk(var, "var")
        if mean.dim() != 2 or var.shape != mean.shape or info.dtype != torch.int32 or info.device != self.device or \
                not info.is_contiguous() or info.numel() != mean.shape[0]:
            raise ValueError("mean and var must be P x T and info P contiguous int32 on %s" % (self.device,))
        P, T = mean.shape
        off = np.asarray(offsets, dtype=np.int64).reshape(-1)
        G = off.size - 1
        if G < 1 or off[0] != 0 or off[-1] != P or np.any(np.diff(off) < 0):
            raise ValueError("offsets must be non-decreasing from 0 to %d (got %d entries)" % (P, off.size))
        if Ytest is not None:
            self._chk(Ytest, "Ytest")
            if tuple(Ytest.shape) != (G, T):
                raise ValueError("Ytest must be %d x %d (got %s)" % (G, T, tuple(Ytest.shape)))
        off_d = torch.as_tensor(off).to(self.device)
        mm, mv = self.empty(G, T), self.empty(G, T)
        lp, mlp = (self.empty(G, T), self.empty(G, T)) if Ytest is not None else (None, None)
        kept = torch.empty(G, dtype=torch.int32, device=self.device)
        lib = self.exact_predict_lib
        ws = self._workspace("exact_mixture", lib.sgp_exact_mixture_workspace_bytes(G, T))
        st = lib.sgp_exact_mixture_reduce(self._ptr(mean), self._ptr(var), self._ptr(info), self._ptr(off_d), G, T, self._ptr(Ytest),
                                          self._ptr(mm), self._ptr(mv), self._ptr(lp), self._ptr(mlp), self._ptr(kept), self._ptr(ws),
                                          ws.numel(), self._stream())
        _lib.check("sgp_exact_mixture_reduce", st)
        return {"mean": mm, "var": mv, "logpdf": lp, "mean_logpdf": mlp, "kept": kept}

    @staticmethod
    def _mixture_quantiles_intake(device, mean, var, info, offsets, probs, Ytest=None):
        """What ``mixture_quantiles`` refuses before it allocates anything: returns (P, T, G, offsets as int64 numpy, probs as a C array
        of Q doubles).  It runs on CPU tensors as well."""
        _chk(device, mean, "mean"), _chk(device, var, "var")
        if mean.dim() != 2 or var.shape != mean.shape or not isinstance(info, torch.Tensor) or info.dtype != torch.int32 or \
                info.device != device or not info.is_contiguous() or info.numel() != mean.shape[0]:
            raise ValueError("mean and var must be P x T and info P contiguous int32 on %s" % (device,))
        P, T = mean.shape
        off = np.asarray(offsets)
        if off.dtype.kind not in "iu" or off.ndim != 1:
            raise ValueError("offsets must be a sequence of integers")
        off = off.astype(np.int64)
        G = off.size - 1
        if G < 1 or off[0] != 0 or off[-1] != P or np.any(np.diff(off) < 0):
            raise ValueError("offsets must be non-decreasing from 0 to %d (got %d entries)" % (P, off.size))
        pr = np.asarray(probs, dtype=np.float64).reshape(-1)
        if not 1 <= pr.size <= _lib.MIXTURE_MAX_Q or not np.all((pr >= _lib.MIXTURE_P_MIN) & (pr <= 1.0 - _lib.MIXTURE_P_MIN)):
            raise ValueError("probs must be 1 to %d probabilities in [%g, 1 - %g] (got %s)"
                             % (_lib.MIXTURE_MAX_Q, _lib.MIXTURE_P_MIN, _lib.MIXTURE_P_MIN, pr.tolist()))
        if Ytest is not None:
            _chk(device, Ytest, "Ytest")
            if tuple(Ytest.shape) != (G, T):
                raise ValueError("Ytest must be %d x %d (got %s)" % (G, T, tuple(Ytest.shape)))
        return P, T, G, off, (C.c_double * pr.size)(*pr.tolist())

    def mixture_quantiles(self, mean, var, info, offsets, probs, Ytest=None, want_iters=False):
        """Quantiles and the PIT of the mixture over the draws of each group in ONE launch (include/sgp_mixture.h:
        sgp_mixture_quantiles), on what ``exact_mixture`` takes: rows [offsets[g], offsets[g + 1]) of mean / var (P x T, device) are the
        draws of group g; draws with info != 0 are left out.  ``probs``: 1 to 8 host probabilities in [1e-9, 1 - 1e-9].  Returns a
        dict of device tensors: quantiles [G, Q, T], pit [G, T] = the mixture CDF at ``Ytest`` (G x T; None without), iters [G, T]
        int32 with ``want_iters`` (None without).  A group with no draw left is NaN.  Nothing is synchronised."""
        _, T, G, off, pr = self._mixture_quantiles_intake(self.device, mean, var, info, offsets, probs, Ytest)
        Q = len(pr)
        off_d = torch.as_tensor(off).to(self.device)
        quant = self.empty(G, Q, T)
        pit = self.empty(G, T) if Ytest is not None else None
        iters = torch.empty(G, T, dtype=torch.int32, device=self.device) if want_iters else None
        lib = self.mixture_lib
        ws = self._workspace("mixture_quantiles", lib.sgp_mixture_quantiles_workspace_bytes(G, T, Q))
        st = lib.sgp_ctx_mixture_quantiles(self._c(), self._ptr(mean), self._ptr(var), self._ptr(info), self._ptr(off_d), G, T, pr, Q,
                                           self._ptr(Ytest), self._ptr(quant), self._ptr(pit), self._ptr(iters), self._ptr(ws),
                                           ws.numel(), self._stream())
        _lib.check("sgp_mixture_quantiles", st)
        return {"quantiles": quant, "pit": pit, "iters": iters}

    def _launch_budget(self, budget: int, lib, occupancy: str, size: int, C: int, kernel) -> int:
        """``budget`` divided by the number of waves of workgroups C chains make on this device (chains per CU from the library's
        ``occupancy`` query at ``size``)."""
        per_cu = int(getattr(lib, occupancy)(int(size), _kernel_id(kernel)))
        _lib.check(occupancy, min(per_cu, 0))
        slots = max(1, per_cu * torch.cuda.get_device_properties(self.device).multi_processor_count)
        return budget // -(-int(C) // slots)

    def _nuts_batch(self, ws_key, ws_bytes, begin, advance, budget, X, Y, Z, idx, limits, q0, seeds, n_tune, n_draws, kernel, jitter,
                    max_treedepth, step_scale, target_accept, evals_per_launch):
        """The driver of the device-resident samplers: the intake of the data, q0 and the seeds, the output buffers, begin, the loop of
        bounded launches with its one 8-byte read-back each, and the host dict.  The caller supplies its library's workspace query
        (cached as ``ws_key``), its ``begin`` and ``advance`` as (name for the status check, bound function) and its default
        ``budget(C, N, M)`` of evaluations per launch; with a Z the C calls carry M and the inducing sets."""
        d = X.shape[-1]
        q0 = torch.as_tensor(np.asarray(q0.cpu() if isinstance(q0, torch.Tensor) else q0, dtype=np.float64)).reshape(-1, d + 2)
        q0 = q0.to(self.device).contiguous()
        C_ = q0.shape[0]
        seeds = np.asarray([int(s) & ((1 << 64) - 1) for s in (seeds.tolist() if hasattr(seeds, "tolist") else seeds)], dtype=np.uint64)
        own = (C_, seeds.size == C_ and n_draws >= 1 and n_tune >= 0,
               ", q0 %s, %d seeds, n_tune %d, n_draws %d" % (tuple(q0.shape), seeds.size, n_tune, n_draws))
        (X, Y, Z, _), idx, (N, d, M, _, _) = self._batch_intake(self.device, X, Y, Z, idx=idx, limits=limits, own=own)
        seeds_d = torch.as_tensor(seeds.view(np.int64)).to(self.device)
        kid = _kernel_id(kernel)
        dims = (C_, N, d) if Z is None else (C_, N, M, d)
        samples, stats, seconds = self.empty(C_, n_draws, d + 2), self.empty(C_, n_draws, 8), self.empty(C_, n_draws)
        counts = torch.empty(2, C_, dtype=torch.int64, device=self.device)
        info = torch.empty(C_, dtype=torch.int32, device=self.device)
        ws = self._workspace(ws_key, ws_bytes(*dims))
        outs = (self._ptr(samples), self._ptr(stats), self._ptr(seconds), self._ptr(counts[0]), self._ptr(counts[1]), self._ptr(info))
        _lib.check(begin[0], begin[1](
            self._c(), self._ptr(q0), self._ptr(seeds_d), *dims, kid, int(n_tune), int(n_draws), int(max_treedepth), float(step_scale),
            float(target_accept), *outs, self._ptr(ws), ws.numel(), self._stream()))
        if evals_per_launch is None:
            evals_per_launch = budget(C_, N, M)
        data = [self._ptr(X), N * d, d, self._ptr(Y), N, self._ptr(idx[0]), self._ptr(idx[1])]
        if Z is not None:
            data += [self._ptr(Z), M * d, d, self._ptr(idx[2])]
        finished, launches = C.c_int64(0), 0
        while finished.value < C_:
            _lib.check(advance[0], advance[1](
                self._c(), *data, *dims, kid, float(jitter), *outs, int(evals_per_launch), C.byref(finished), self._ptr(ws), ws.numel(),
                self._stream()))
            launches += 1
        counts = counts.to("cpu")
        return {"samples": samples.to("cpu"), "stats": stats.to("cpu"), "seconds": seconds.to("cpu"), "evaluations": counts[0],
                "draws": counts[1], "info": info.to("cpu"), "launches": launches}

    # Evaluations one resident workgroup runs back to back in a launch of ``exact_nuts_batch`` by default (1024 x the
    # measured 138 us per evaluation of one chain at N = 128 keeps the longest launch near 0.14 s); shared among the waves of workgroups
    # when there are more chains than the chip holds at a time.
    EXACT_NUTS_LAUNCH_EVALS = 1024

    def exact_nuts_evals_per_launch(self, C: int, N: int, kernel="rbf") -> int:
        """The default ``evals_per_launch`` of ``exact_nuts_batch``: ``EXACT_NUTS_LAUNCH_EVALS`` divided by the number of waves of
        workgroups C chains make on this device (chains per CU from ``sgp_exact_nuts_batch_occupancy``)."""
        return max(1, self._launch_budget(self.EXACT_NUTS_LAUNCH_EVALS, self.exact_nuts_lib, "sgp_exact_nuts_batch_occupancy", N, C, kernel))

    def exact_nuts_batch(self, X, Y, q0, seeds, n_tune, n_draws, ix=None, iy=None, kernel="rbf", jitter=0.0, max_treedepth=10,
                         step_scale=0.25, target_accept=0.8, evals_per_launch=None):
        """C independent NUTS chains over the exact marginal likelihood, one workgroup each, entirely on the device (include/sgp_exact_nuts.h:
        sgp_exact_nuts_batch_begin / _advance).  X: nX x N x d (or N x d), Y: nY x N (or N) -- device tensors; chain c samples data set
        ix[c] with target iy[c] (None: set 0) from q0[c] (C x (d + 2), unconstrained) with the splitmix64 stream of seeds[c].  The run is
        a loop of bounded launches (``evals_per_launch`` evaluations per chain each, default ``exact_nuts_evals_per_launch``) with one
        8-byte read-back per launch; no output but ``seconds`` depends on how it is cut.  Returns host tensors: samples [C, n_draws,
        d + 2], stats [C, n_draws, 8], seconds [C, n_draws], evaluations [C], draws [C] (int64), info [C] (int32: 0, or
        ``_lib.EXACT_NUTS_BAD_START`` -- no finite density at the start, that chain's rows are NaN), and ``launches``."""
        lib = self.exact_nuts_lib
        return self._nuts_batch(
            "exact_nuts", lib.sgp_exact_nuts_batch_workspace_bytes, ("sgp_exact_nuts_batch_begin", lib.sgp_ctx_exact_nuts_batch_begin),
            ("sgp_exact_nuts_batch_advance", lib.sgp_ctx_exact_nuts_batch_advance), lambda C_, N, M: self.exact_nuts_evals_per_launch(C_, N, kernel),
            X, Y, None, (ix, iy), None, q0, seeds, n_tune, n_draws, kernel, jitter, max_treedepth, step_scale, target_accept, evals_per_launch)

    # Row tiles one resident workgroup walks in a launch of ``vfe_nuts_batch`` by default (an evaluation walks
    # vb_tiles(N, Mp) row tiles twice and costs at most 24 us per tile in the single-workgroup rows of profiles/vfe_batch_rates.json,
    # so 4096 tiles keep the longest launch near 0.1 s -- derived from those rows, not fitted to the sampler, whose launches then
    # measured 60 to 80 ms in profiles/vfe_nuts_rates.json); shared among the waves of workgroups when there are more chains than the
    # chip holds at a time.
    VFE_NUTS_LAUNCH_TILES = 4096

    @staticmethod
    def _vfe_tiles(N: int, M: int) -> int:
        """vb_tiles(N, Mp) of csrc/sgp_vfe_batch.hpp: the row tiles (2048 / Mp rows each, Mp the size class of M) that cover N rows."""
        rows = 2048 // (16 if M <= 16 else 32 if M <= 32 else 64)
        return -(-int(N) // rows)

    def vfe_nuts_evals_per_launch(self, C: int, N: int, M: int, kernel="rbf") -> int:
        """The default ``evals_per_launch`` of ``vfe_nuts_batch``: ``VFE_NUTS_LAUNCH_TILES`` divided by the number of waves of workgroups
        C chains make on this device (chains per CU from ``sgp_vfe_nuts_batch_occupancy``), in evaluations of ``vb_tiles(N, Mp)`` row
        tiles each; never below 1."""
        tiles = self._launch_budget(self.VFE_NUTS_LAUNCH_TILES, self.vfe_nuts_lib, "sgp_vfe_nuts_batch_occupancy", M, C, kernel)
        return max(1, tiles // self._vfe_tiles(N, M))

    def vfe_nuts_batch(self, X, Y, Z, q0, seeds, n_tune, n_draws, ix=None, iy=None, iz=None, kernel="rbf", jitter=1e-6, max_treedepth=10,
                       step_scale=0.25, target_accept=0.8, evals_per_launch=None):
        """C independent NUTS chains over the collapsed (VFE) bound at fixed inducing inputs, one workgroup each, entirely on the device
        (include/sgp_vfe_nuts.h: sgp_vfe_nuts_batch_begin / _advance).  X: nX x N x d (or N x d), Y: nY x N (or N), Z: nZ x M x d (or
        M x d) -- device tensors; chain c samples data set ix[c] with target iy[c] and inducing set iz[c] (None: set 0) from q0[c]
        (C x (d + 2), unconstrained) with the splitmix64 stream of seeds[c]; ``jitter`` goes on K_uu.  The run is a loop of bounded
        launches (``evals_per_launch`` evaluations per chain each, default ``vfe_nuts_evals_per_launch``) with one 8-byte read-back per
        launch; no output but ``seconds`` depends on how it is cut.  Returns host tensors: samples [C, n_draws, d + 2], stats [C,
        n_draws, 8], seconds [C, n_draws], evaluations [C], draws [C] (int64), info [C] (int32: 0, or ``_lib.VFE_NUTS_BAD_START`` -- no
        finite density at the start, that chain's rows are NaN), and ``launches``."""
        lib = self.vfe_nuts_lib
        return self._nuts_batch(
            "vfe_nuts", lib.sgp_vfe_nuts_batch_workspace_bytes, ("sgp_vfe_nuts_batch_begin", lib.sgp_ctx_vfe_nuts_batch_begin),
            ("sgp_vfe_nuts_batch_advance", lib.sgp_ctx_vfe_nuts_batch_advance), lambda C_, N, M: self.vfe_nuts_evals_per_launch(C_, N, M, kernel),
            X, Y, Z, (ix, iy, iz), ("vfe_nuts_batch", "C"), q0, seeds, n_tune, n_draws, kernel, jitter, max_treedepth, step_scale,
            target_accept, evals_per_launch)

    def exact_predict(self, Xs, X, ls, sf2, s2, factors, kernel="rbf", pred_noise=True, full_cov=False):
        """Exact posterior predictive at the rows of Xs from ``exact_eval(..., want_factors=True)``'s factors at the same (X, theta)
        (include/sgp.h: sgp_exact_predict).  Returns (mean, var, cov or None) as device tensors; nothing is synchronised."""
        T, d = Xs.shape
        N = X.shape[0]
        self._chk(Xs, "Xs"), self._chk(X, "X"), self._chk(factors, "factors")
        mean, var = self.empty(T), self.empty(T)
        cov = self.empty(T, T) if full_cov else None
        ws = self._workspace("exact_predict", self.lib.sgp_exact_predict_workspace_bytes(T, N, d, 1 if full_cov else 0))
        st = self.lib.sgp_ctx_exact_predict(
            self._c(), self._ptr(Xs), d, T, self._ptr(X), d, N, d, self._inv_ls(ls, d, kernel), float(sf2), float(s2), self._ptr(factors),
            _kernel_id(kernel), 1 if pred_noise else 0, self._ptr(mean), self._ptr(var), self._ptr(cov), self._ptr(ws), ws.numel(),
            self._stream())
        _lib.check("sgp_exact_predict", st)
        return mean, var, cov

    # ------------------------------------------------------------------ SVGP minibatch bound
    def svgp_elbo(self, Xb, yb, Z, ls, sf2, s2, m, LS, N_total, jitter=1e-6, kernel="rbf", likelihood="gaussian",
                  with_grads=False):
        """One minibatch of the whitened SVGP bound.  Returns dict(out=[elbo/datum, sum ELL, KL], info, and with
        ``with_grads`` g_m, g_LS (lower), g_Z, g_ls, g_sf2, g_s2 as device tensors).  Nothing is synchronised."""
        B, d = Xb.shape
        M = Z.shape[0]
        for t, n in ((Xb, "Xb"), (yb, "yb"), (Z, "Z"), (m, "m"), (LS, "LS")):
            self._chk(t, n)
        lik = _likelihood_id(likelihood)
        out = self.empty(3)
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        res = {"out": out, "info": info}
        g = {}
        if with_grads:
            g = {"g_m": self.empty(M), "g_LS": self.empty(M, M), "g_Z": self.empty(M, d), "g_ls": self.empty(d),
                 "g_sf2": self.empty(1), "g_s2": self.empty(1)}
            res.update(g)
        nbytes = self.lib.sgp_svgp_workspace_bytes(B, M, d)
        if nbytes == 0:
            raise ValueError("unsupported SVGP shape B=%d M=%d d=%d" % (B, M, d))
        ws = self._workspace("svgp", nbytes)
        st = self._cf.sgp_svgp_elbo(
            self._ptr(Xb), d, self._ptr(yb), B, self._ptr(Z), d, self._inv_ls(ls, d), float(sf2), float(s2), float(jitter),
            self._ptr(m), self._ptr(LS), int(N_total), M, d, _kernel_id(kernel), lik, 1 if with_grads else 0, self._ptr(out),
            self._ptr(g.get("g_m")), self._ptr(g.get("g_LS")), self._ptr(g.get("g_Z")), self._ptr(g.get("g_ls")),
            self._ptr(g.get("g_sf2")), self._ptr(g.get("g_s2")), self._ptr(info), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_svgp_elbo", st)
        return res

    def svgp_elbo_batch(self, Xb, yb, Z, ls, sf2, s2, m, LS, N_total, jitter=1e-6, kernel="rbf", likelihood="gaussian",
                        with_grads=False, defer_reverse=False):
        """The bound of one minibatch at S hyper-parameter samples in ONE chain of launches (sgp_svgp_elbo_batch).
        ls: S x d, sf2, s2: S (host sequences / arrays).  Returns dict(out [S, 4] = [bound per datum | sum E log p | KL | status], info [S], and with ``with_grads``
        g_m [S, M], g_LS [S, M, M], g_Z [S, M, d], g_ls [S, d], g_sf2 [S], g_s2 [S]); device tensors, nothing synchronised."""
        import ctypes
        B, d = Xb.shape
        M = Z.shape[0]
        for t, n in ((Xb, "Xb"), (yb, "yb"), (Z, "Z"), (m, "m"), (LS, "LS")):
            self._chk(t, n)
        lsv = [[float(v) for v in row] for row in ls]
        S = len(lsv)
        if any(len(row) != d for row in lsv) or len(sf2) != S or len(s2) != S:
            raise ValueError("ls must be S x d, sf2 and s2 of length S")
        lik = _likelihood_id(likelihood)
        inv = (ctypes.c_double * (S * d))(*[1.0 / v for row in lsv for v in row])
        sf2c = (ctypes.c_double * S)(*[float(v) for v in sf2])
        s2c = (ctypes.c_double * S)(*[float(v) for v in s2])
        out = self.empty(S, 4)
        info = torch.empty(S, dtype=torch.int32, device=self.device)
        res = {"out": out, "info": info}
        g = {}
        if with_grads:
            g = {"g_m": self.empty(S, M), "g_LS": self.empty(S, M, M), "g_Z": self.empty(S, M, d), "g_ls": self.empty(S, d),
                 "g_sf2": self.empty(S), "g_s2": self.empty(S)}
            res.update(g)
        nbytes = self.lib.sgp_svgp_batch_workspace_bytes(B, M, d, S)
        if nbytes == 0:
            raise ValueError("unsupported SVGP batch shape B=%d M=%d d=%d S=%d (S <= 8)" % (B, M, d, S))
        ws = self._workspace("svgp_batch", nbytes)
        if with_grads and defer_reverse:
            # two halves: the forward now; res["reverse"]() enqueues the reverse chain (the caller copies the bounds out in
            # between, so that they reach the host while the device is still busy with the gradients)
            head = (self._ptr(Xb), d, self._ptr(yb), B, self._ptr(Z), d, S, inv, sf2c, s2c, float(jitter), self._ptr(m), self._ptr(LS),
                    int(N_total), M, d, _kernel_id(kernel), lik)
            st = self._cf.sgp_svgp_elbo_batch_forward(*head, self._ptr(out), self._ptr(g["g_s2"]), self._ptr(info), self._ptr(ws),
                                                      ws.numel(), self._stream())
            _lib.check("sgp_svgp_elbo_batch_forward", st)
            keep = (Xb, yb, Z, m, LS, ws)  # the buffers the deferred call reads

            def reverse():
                st2 = self._cf.sgp_svgp_elbo_batch_reverse(*head, self._ptr(g["g_m"]), self._ptr(g["g_LS"]), self._ptr(g["g_Z"]),
                                                           self._ptr(g["g_ls"]), self._ptr(g["g_sf2"]), self._ptr(keep[5]), keep[5].numel(),
                                                           self._stream())
                _lib.check("sgp_svgp_elbo_batch_reverse", st2)

            res["reverse"] = reverse
            return res
        st = self._cf.sgp_svgp_elbo_batch(
            self._ptr(Xb), d, self._ptr(yb), B, self._ptr(Z), d, S, inv, sf2c, s2c, float(jitter), self._ptr(m), self._ptr(LS),
            int(N_total), M, d, _kernel_id(kernel), lik, 1 if with_grads else 0, self._ptr(out),
            self._ptr(g.get("g_m")), self._ptr(g.get("g_LS")), self._ptr(g.get("g_Z")), self._ptr(g.get("g_ls")),
            self._ptr(g.get("g_sf2")), self._ptr(g.get("g_s2")), self._ptr(info), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_svgp_elbo_batch", st)
        return res

    def svgp_predict_batch(self, Xs, Z, ls, sf2, m, LS, jitter=1e-6, kernel="rbf"):
        """q(f*) at the rows of Xs for S hyper-parameter samples (ls: S x d, sf2: S), eight per chain of launches.
        Returns (mean [S, T], var [S, T], info [S] int32) on the device."""
        import ctypes
        T, d = Xs.shape
        M = Z.shape[0]
        lsv = [[float(v) for v in row] for row in ls]
        S = len(lsv)
        mean, var = self.empty(S, T), self.empty(S, T)
        info = torch.zeros(S, dtype=torch.int32, device=self.device)
        # test rows in chunks: the library carves S x 6 x Mp x Tp doubles for its "minibatch" -- 10 GB at S = 8,
        # M = 512, T = 50k in one piece, and T > 2^20 is refused outright; 8192 rows at a time as sgp_mixture_predict does
        TC = self.SVGP_PREDICT_CHUNK
        for s0 in range(0, S, 8):
            n = min(8, S - s0)
            inv = (ctypes.c_double * (n * d))(*[1.0 / v for row in lsv[s0:s0 + n] for v in row])
            sf2c = (ctypes.c_double * n)(*[float(v) for v in sf2[s0:s0 + n]])
            for t0 in range(0, T, TC):
                tn = min(TC, T - t0)
                nbytes = self.lib.sgp_svgp_batch_workspace_bytes(tn, M, d, n)
                if nbytes == 0:
                    raise ValueError("unsupported SVGP predictive shape T=%d M=%d d=%d" % (T, M, d))
                ws = self._workspace("svgp_batch", nbytes)
                whole = tn == T
                mc, vc = (mean[s0:s0 + n], var[s0:s0 + n]) if whole else (self.empty(n, tn), self.empty(n, tn))
                ic = info[s0:s0 + n] if whole else torch.empty(n, dtype=torch.int32, device=self.device)
                st = self._cf.sgp_svgp_predict_batch(self._ptr(Xs[t0:t0 + tn]), d, tn, self._ptr(Z), d, n, inv, sf2c, float(jitter),
                                                     self._ptr(m), self._ptr(LS), M, d, _kernel_id(kernel), self._ptr(mc), self._ptr(vc),
                                                     C.c_void_p(ic.data_ptr()), self._ptr(ws), ws.numel(), self._stream())
                _lib.check("sgp_svgp_predict_batch", st)
                if not whole:
                    mean[s0:s0 + n, t0:t0 + tn] = mc
                    var[s0:s0 + n, t0:t0 + tn] = vc
                    info[s0:s0 + n] = torch.where(info[s0:s0 + n] != 0, info[s0:s0 + n], ic)  # the first failure stays
        return mean, var, info

    SVGP_PREDICT_CHUNK = 8192  # test rows per sgp_svgp_predict_batch call

    def svgp_batch_combine(self, res, weights):
        """Reverse pass of sum_s weights[s] * bound_s from a ``svgp_elbo_batch(..., with_grads=True)`` result, one launch.
        Returns (g_m [M], g_LS [M, M], g_Z [M, d], g_theta [S, d + 2] = w_s [d/dsf2 | d/dls | d/ds2]) on the device."""
        import ctypes
        S, M, d = res["g_Z"].shape
        w = (ctypes.c_double * S)(*[float(v) for v in weights])
        gm, gLS, gZ, gth = self.empty(M), self.empty(M, M), self.empty(M, d), self.empty(S, d + 2)
        st = self.lib.sgp_svgp_batch_combine(S, w, M, d, self._ptr(res["g_m"]), self._ptr(res["g_LS"]), self._ptr(res["g_Z"]),
                                             self._ptr(res["g_ls"]), self._ptr(res["g_sf2"]), self._ptr(res["g_s2"]), self._ptr(gm),
                                             self._ptr(gLS), self._ptr(gZ), self._ptr(gth), self._stream())
        _lib.check("sgp_svgp_batch_combine", st)
        return gm, gLS, gZ, gth

    MIXTURE_BATCH = 8  # hyper-parameter samples per sgp_mixture_predict call

    def mixture_predict(self, X, y, Xs, Z, ls, sf2, s2, jitter=1e-6, kernel="rbf", pred_noise=True, full_cov=False, gate_jitter=None):
        """Predictive of the collapsed bound at S hyper-parameter samples (ls: S x d, sf2, s2: S host sequences; Z: M x d, or S x M x d
        for inducing inputs of their own per sample -- all_in_HMC's draws, sgp_mixture_predict_zs), eight samples
        per chain of launches.  Returns dict(mean [S, T], var [S, T], cov [S, T, T] or None, info [S] int32, gate [S] int32 or
        None: status of cholesky(cov + gate_jitter I), the reference's PSD gate) -- device tensors, nothing synchronised."""
        import ctypes
        N, d = X.shape
        T = Xs.shape[0]
        per_z = Z.dim() == 3  # (S, M, d): inducing inputs of their own for every sample (sgp_mixture_predict_zs)
        M = Z.shape[-2]
        for t, n in ((X, "X"), (y, "y"), (Xs, "Xs"), (Z, "Z")):
            self._chk(t, n)
        lsv = [[float(v) for v in row] for row in ls]
        S = len(lsv)
        if per_z and (Z.shape[0] != S or Z.shape[2] != d):
            raise ValueError("a per-sample Z must be S x M x d")
        if any(len(row) != d for row in lsv) or len(sf2) != S or len(s2) != S:
            raise ValueError("ls must be S x d, sf2 and s2 of length S")
        want_gate = full_cov and gate_jitter is not None
        mean, var = self.empty(S, T), self.empty(S, T)
        cov = self.empty(S, T, T) if full_cov else None
        info = torch.empty(S, dtype=torch.int32, device=self.device)
        gate = torch.empty(S, dtype=torch.int32, device=self.device) if want_gate else None
        for s0 in range(0, S, self.MIXTURE_BATCH):
            n = min(self.MIXTURE_BATCH, S - s0)
            nbytes = self.lib.sgp_mixture_predict_workspace_bytes(N, T, M, d, n, 1 if full_cov else 0, 1 if want_gate else 0)
            if nbytes == 0:
                raise ValueError("unsupported mixture-predictive shape N=%d T=%d M=%d d=%d (full covariance needs T <= 8192)" % (N, T, M, d))
            ws = self._workspace("mixture", nbytes)
            inv = (ctypes.c_double * (n * d))(*[1.0 / v for row in lsv[s0:s0 + n] for v in row])
            sf2c = (ctypes.c_double * n)(*[float(v) for v in sf2[s0:s0 + n]])
            s2c = (ctypes.c_double * n)(*[float(v) for v in s2[s0:s0 + n]])
            zargs = (C.c_void_p(Z.data_ptr() + 8 * s0 * M * d), d, M * d) if per_z else (self._ptr(Z), d)
            fn = self.lib.sgp_ctx_mixture_predict_zs if per_z else self.lib.sgp_ctx_mixture_predict
            st = fn(
                self._c(), self._ptr(X), d, self._ptr(y), N, self._ptr(Xs), d, T, *zargs, n, inv, sf2c, s2c, float(jitter), M, d,
                _kernel_id(kernel), 1 if pred_noise else 0, float(gate_jitter) if want_gate else 0.0, self._ptr(mean[s0:]), self._ptr(var[s0:]),
                self._ptr(cov[s0:]) if full_cov else None, C.c_void_p(info[s0:].data_ptr()),
                C.c_void_p(gate[s0:].data_ptr()) if want_gate else None, self._ptr(ws), ws.numel(), self._stream())
            _lib.check("sgp_mixture_predict_zs" if per_z else "sgp_mixture_predict", st)
        return {"mean": mean, "var": var, "cov": cov, "info": info, "gate": gate}

    def svgp_predict(self, Xs, Z, ls, sf2, m, LS, jitter=1e-6, kernel="rbf"):
        T, d = Xs.shape
        M = Z.shape[0]
        mean, var = self.empty(T), self.empty(T)
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        ws = self._workspace("svgp", self.lib.sgp_svgp_workspace_bytes(T, M, d))
        st = self._cf.sgp_svgp_predict(self._ptr(Xs), d, T, self._ptr(Z), d, self._inv_ls(ls, d), float(sf2), float(jitter),
                                       self._ptr(m), self._ptr(LS), M, d, _kernel_id(kernel), self._ptr(mean), self._ptr(var),
                                       self._ptr(info), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_svgp_predict", st)
        return mean, var, info

    # ------------------------------------------------------------------ multi-class (robust-max) SVGP bound
    def svgp_mc_elbo(self, Xb, yb, Z, ls, sf2, m, LS, N_total, eps=1e-3, jitter=1e-6, kernel="rbf", with_grads=False):
        """One minibatch of the multi-class SVGP bound (include/sgp.h: sgp_svgp_mc_elbo).  ``yb``: labels 0 .. C-1 as doubles, ``m``: C x M,
        ``LS``: C x M x M on the device.  Returns dict(out [4] = [bound per datum | sum E log p | KL | status word], info, and with
        ``with_grads`` g_m [C, M], g_LS [C, M, M], g_Z [M, d], g_ls [d], g_sf2 [1]); device tensors, nothing synchronised."""
        B, d = Xb.shape
        Cn, M = m.shape
        if LS.shape != (Cn, M, M) or Z.shape != (M, d):
            raise ValueError("svgp_mc_elbo: m is C x M, LS is C x M x M, Z is M x d")
        for t, n in ((Xb, "Xb"), (yb, "yb"), (Z, "Z"), (m, "m"), (LS, "LS")):
            self._chk(t, n)
        out = self.empty(4)
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        res = {"out": out, "info": info}
        g = {}
        if with_grads:
            g = {"g_m": self.empty(Cn, M), "g_LS": self.empty(Cn, M, M), "g_Z": self.empty(M, d), "g_ls": self.empty(d),
                 "g_sf2": self.empty(1)}
            res.update(g)
        nbytes = self.lib.sgp_svgp_mc_workspace_bytes(B, M, d, Cn)
        if nbytes == 0:
            raise ValueError("unsupported multi-class SVGP shape B=%d M=%d d=%d C=%d" % (B, M, d, Cn))
        ws = self._workspace("svgp_mc", nbytes)
        st = self._cf.sgp_svgp_mc_elbo(
            self._ptr(Xb), d, self._ptr(yb), B, self._ptr(Z), d, self._inv_ls(ls, d), float(sf2), float(jitter), self._ptr(m),
            self._ptr(LS), Cn, float(eps), int(N_total), M, d, _kernel_id(kernel), 1 if with_grads else 0, self._ptr(out),
            self._ptr(g.get("g_m")), self._ptr(g.get("g_LS")), self._ptr(g.get("g_Z")), self._ptr(g.get("g_ls")),
            self._ptr(g.get("g_sf2")), self._ptr(info), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_svgp_mc_elbo", st)
        return res

    SVGP_MC_PREDICT_CHUNK = 4096  # test rows per sgp_svgp_mc_predict call (the workspace holds C x Mp x rows)

    def svgp_mc_predict(self, Xs, Z, ls, sf2, m, LS, eps=1e-3, jitter=1e-6, kernel="rbf", want_probs=True):
        """Latent means and variances (T x C each) of the C classes at the rows ``Xs`` and, with ``want_probs``, the class probabilities
        (T x C) of the robust-max likelihood, all formed on the device (sgp_svgp_mc_predict).  Returns (mean, var, probs or None, info)."""
        T, d = Xs.shape
        Cn, M = m.shape
        for t, n in ((Xs, "Xs"), (Z, "Z"), (m, "m"), (LS, "LS")):
            self._chk(t, n)
        mean, var = self.empty(T, Cn), self.empty(T, Cn)
        probs = self.empty(T, Cn) if want_probs else None
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        for t0 in range(0, T, self.SVGP_MC_PREDICT_CHUNK):
            tn = min(self.SVGP_MC_PREDICT_CHUNK, T - t0)
            nbytes = self.lib.sgp_svgp_mc_workspace_bytes(tn, M, d, Cn)
            if nbytes == 0:
                raise ValueError("unsupported multi-class SVGP shape T=%d M=%d d=%d C=%d" % (tn, M, d, Cn))
            ws = self._workspace("svgp_mc", nbytes)
            mc, vc = self.empty(Cn, tn), self.empty(Cn, tn)
            st = self._cf.sgp_svgp_mc_predict(
                self._ptr(Xs[t0:t0 + tn]), d, tn, self._ptr(Z), d, self._inv_ls(ls, d), float(sf2), float(jitter), self._ptr(m),
                self._ptr(LS), Cn, float(eps), M, d, _kernel_id(kernel), self._ptr(mc), self._ptr(vc),
                self._ptr(probs[t0:t0 + tn]) if want_probs else None, self._ptr(info), self._ptr(ws), ws.numel(), self._stream())
            _lib.check("sgp_svgp_mc_predict", st)
            mean[t0:t0 + tn] = mc.T
            var[t0:t0 + tn] = vc.T
        return mean, var, probs, info  # every chunk factors the same K_uu: one status word says it all

    # ------------------------------------------------------------------ stand-alone M x M entry points
    def chol_lower(self, A: torch.Tensor):
        M = A.shape[0]
        A = A.clone().contiguous()
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        ws = self._workspace("chol", self.lib.sgp_chol_workspace_bytes(M))
        st = self._cf.sgp_chol_lower(self._ptr(A), M, M, self._ptr(info), self._ptr(ws), ws.numel(), self._stream())
        _lib.check("sgp_chol_lower", st)
        return A, info

    def trsm_lower(self, L: torch.Tensor, B: torch.Tensor, trans=False):
        M, k = B.shape
        B = B.clone().contiguous()
        ws = self._workspace("trsm", self.lib.sgp_trsm_workspace_bytes(M, k))
        st = self._cf.sgp_trsm_lower(self._ptr(L), M, self._ptr(B), k, 1 if trans else 0, M, k, self._ptr(ws), ws.numel(),
                                     self._stream())
        _lib.check("sgp_trsm_lower", st)
        return B

    def logdiag_sum(self, L: torch.Tensor):
        out = self.empty(1)
        st = self.lib.sgp_logdiag_sum(self._ptr(L), L.shape[1], L.shape[0], self._ptr(out), self._stream())
        _lib.check("sgp_logdiag_sum", st)
        return out
