"""ctypes binding of libsgp_hip.so -- one Python prototype per entry point of include/sgp.h.

There is deliberately no fallback: if the HIP library is missing or does not export a symbol the
import fails loudly (``SgpLibraryError``).  The product path never computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libsgp_hip.so")

SGP_ABI_VERSION = 3
SGP_MAX_DIM = 32
SGP_MAX_INDUCING = 4096
KERNEL_IDS = {"rbf": 0, "matern32": 1, "matern52": 2, "composite": 3}
LIKELIHOOD_IDS = {"gaussian": 0, "bernoulli": 1, "bernoulli_logit": 2, "poisson": 3}  # SGP_LIK_* ("bernoulli" = the probit link)
SGPMC_LIK_OUT_LEN = 3
SGP_LIK_MULTICLASS_ROBUSTMAX = 4   # no likelihood_id argument takes it: sgp_sgpmc_mc_rows / sgp_sgpmc_mc_tail serve it
SGP_MAX_CLASSES = 16
COMP_LEN = 33  # SGP_COMP_LEN: doubles in a composite-kernel parameter block (include/sgp.h)
OPT_CONTRACTION, OPT_ASM_OVERLAP, OPT_KFU_BUDGET_BYTES, OPT_COND_LIMIT, OPT_CU_BUDGET, OPT_TIMING, OPT_SHARED_DEVICE = range(7)
OUT_F, OUT_LOGMARG, OUT_TRACE, OUT_LOGDETB, OUT_QUAD, OUT_TRW, OUT_S2BAR, OUT_KAPPABAR, OUT_LEN = range(9)


class SgpLibraryError(RuntimeError):
    pass


class SgpStatusError(RuntimeError):
    def __init__(self, fn, status, text):
        super().__init__("%s returned %d: %s" % (fn, status, text))
        self.status = status


_vp, _i64, _i32, _dbl, _sz = C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_size_t
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

_EN_BEGIN = [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
_EN_ADVANCE = [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _sz, _vp]
EXACT_NUTS_BAD_START = 1  # SGP_EXACT_NUTS_BAD_START

# name -> (restype, argtypes) ; mirrors include/sgp.h line by line
PROTOTYPES = {
    "sgp_abi_version": (_i32, []),
    "sgp_status_string": (C.c_char_p, [_i32]),
    # contexts (ABI version 2): first argument = sgp_ctx* (NULL = the default context)
    "sgp_ctx_create": (_vp, [_i32]),
    "sgp_ctx_destroy": (None, [_vp]),
    "sgp_ctx_device": (_i32, [_vp]),
    "sgp_ctx_set_option": (_i32, [_vp, _i32, _dbl]),
    "sgp_ctx_get_option": (_dbl, [_vp, _i32]),
    "sgp_ctx_bind_thread": (None, [_vp]),
    "sgp_ctx_set_pass1_gate": (None, [_vp, _vp]),
    "sgp_ctx_contraction_last": (_i32, [_vp]),
    "sgp_ctx_contraction_would_use_i8": (_i32, [_vp, _i64, _i32]),
    "sgp_ctx_timing_last_ms": (_i32, [_vp, _i32, C.POINTER(C.c_float)]),
    "sgp_ctx_timing_last_rows": (_i64, [_vp, _i32]),
    "sgp_ctx_suffstats_workspace_bytes": (_sz, [_vp, _i64, _i32, _i32, _i32]),
    "sgp_ctx_suffstats_fwd": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_suffstats_bwd": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _dp, _dbl, _vp, _vp, _dbl, _vp, _i64, _i32, _i32, _i32,
                                     _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_kuu_factor": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_kuu_factor_ex": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_bound_from_stats": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _dbl, _i64, _i32, _i32, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # ABI version 3: the guard's fallback orders, the factored pass 2 and the whitened bound with a context
    "sgp_ctx_suffstats_whitened_workspace_bytes": (_sz, [_vp, _i64, _i32, _i32]),
    "sgp_ctx_suffstats_fwd_whitened": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32, _vp,
                                              _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_suffstats_whitened_rows_workspace_bytes": (_sz, [_vp, _i64, _i32, _i32, _i32]),
    "sgp_ctx_suffstats_fwd_whitened_rows": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32, _vp,
                                                   _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_suffstats_extended_workspace_bytes": (_sz, [_vp, _i64, _i32, _i32]),
    "sgp_ctx_suffstats_fwd_extended": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32, _vp, _i32,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_suffstats_fwd_extended_f16": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32, _vp, _i32,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_suffstats_bwd_factored_workspace_bytes": (_sz, [_vp, _i64, _i32, _i32, _i32]),
    "sgp_ctx_suffstats_bwd_factored": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _dp, _dbl, _vp, _vp, _dbl, _vp, _dbl, _i64, _i32, _i32, _i32,
                                              _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_bound_from_whitened_stats": (_i32, [_vp, _vp, _vp, _vp, _vp, _dbl, _i64, _i32, _i32, _vp,
                                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_mixture_predict": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i32, _dp, _dp, _dp, _dbl, _i32, _i32, _i32, _i32,
                                       _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_mixture_predict_zs": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _dp, _dp, _dp, _dbl, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_timing_enable": (None, [_i32]),
    "sgp_timing_last_ms": (_i32, [_i32, C.POINTER(C.c_float)]),
    "sgp_timing_last_rows": (_i64, [_i32]),
    "sgp_set_asm_overlap": (None, [_i32]),
    "sgp_set_cond_limit": (None, [_dbl]),
    "sgp_suffstats_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_suffstats_workspace_bytes_ex": (_sz, [_i64, _i32, _i32, _i32]),
    "sgp_suffstats_bwd_workspace_bytes_ex": (_sz, [_i64, _i32, _i32, _i32]),
    "sgp_kfu_len": (_sz, [_i64, _i32]),
    "sgp_set_kfu_budget_bytes": (None, [_sz]),
    "sgp_set_contraction": (_i32, [_i32]),
    "sgp_contraction_last": (_i32, []),
    "sgp_set_pass1_gate": (None, [_vp]),
    "sgp_suffstats_fwd": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32,
                                 _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_stats_packed_len": (_sz, [_i32]),
    "sgp_stats_pack_lower": (_i32, [_vp, _i32, _vp, _vp]),
    "sgp_stats_unpack_lower": (_i32, [_vp, _i32, _vp, _vp]),
    "sgp_kuu": (_i32, [_vp, _i64, _dp, _dbl, _dbl, _i32, _i32, _i32, _vp, _vp]),
    "sgp_chol_workspace_bytes": (_sz, [_i32]),
    "sgp_chol_lower": (_i32, [_vp, _i64, _i32, _vp, _vp, _sz, _vp]),
    "sgp_trsm_workspace_bytes": (_sz, [_i32, _i32]),
    "sgp_trsm_lower": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp, _sz, _vp]),
    "sgp_logdiag_sum": (_i32, [_vp, _i64, _i32, _vp, _vp]),
    "sgp_bound_workspace_bytes": (_sz, [_i32, _i32]),
    "sgp_bound_factors_len": (_sz, [_i32]),
    "sgp_kuu_inverse_trace_len": (_sz, []),
    "sgp_kuu_inverse_trace": (_i32, [_vp, _i32, _vp, _vp]),
    "sgp_streaming_error_estimate": (_i32, [_vp, _vp, _dbl, _i64, _i32, _vp, _vp]),
    "sgp_streaming_error_bound": (_i32, [_vp, _dbl, _dbl, _vp, _vp]),
    "sgp_streaming_error_report": (_i32, [_vp, _i64, _vp, _dbl, _dbl, _i64, _i32, _vp, _vp]),
    "sgp_kuu_factor_len": (_sz, [_i32]),
    "sgp_kuu_factor_workspace_bytes": (_sz, [_i32]),
    "sgp_kuu_factor": (_i32, [_vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "sgp_kuu_factor_ex": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_bound_from_stats": (_i32, [_vp, _vp, _vp, _vp, _vp, _dbl, _i64, _i32, _i32, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_suffstats_whitened_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_suffstats_fwd_whitened": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32, _vp,
                                          _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_suffstats_whitened_rows_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "sgp_suffstats_fwd_whitened_rows": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32, _vp,
                                               _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_suffstats_extended_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_suffstats_fwd_extended": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32, _vp, _i32,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_suffstats_fwd_extended_ex": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32, _vp, _i32,
                                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_phibar_dd_workspace_bytes": (_sz, [_i32]),
    "sgp_phibar_dd": (_i32, [_vp, _vp, _i32, _dbl, _vp, _vp, _vp, _sz, _vp]),
    "sgp_suffstats_bwd_lo_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_suffstats_bwd_lo": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_suffstats_bwd_lo_workspace_bytes_ex": (_sz, [_i64, _i32, _i32, _i32]),
    "sgp_suffstats_bwd_lo_f16": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_suffstats_fwd_extended_f16": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _i64, _i32, _i32, _i32, _vp, _i32,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_bound_from_whitened_stats": (_i32, [_vp, _vp, _vp, _vp, _dbl, _i64, _i32, _i32, _vp,
                                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_bound_from_whitened_stats_ex": (_i32, [_vp, _vp, _vp, _vp, _dbl, _i64, _i32, _i32, _vp,
                                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # SGPMC: the joint density of the whitened inducing values and the data, from the whitened statistics
    "sgp_sgpmc_workspace_bytes": (_sz, [_i32]),
    "sgp_sgpmc_from_whitened_stats": (_i32, [_vp, _vp, _vp, _vp, _vp, _dbl, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # ... with a non-conjugate likelihood: the row pass over T = K'_fu L^-T and its M x M tail
    "sgp_sgpmc_lik_rows_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_sgpmc_lik_rows": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _dbl, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32,
                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_sgpmc_lik_workspace_bytes": (_sz, [_i32]),
    "sgp_sgpmc_lik_tail": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # ... with the multi-class robust-max likelihood: C latent GPs, V is C x M
    "sgp_sgpmc_mc_rows_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "sgp_sgpmc_mc_rows": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _vp, _i32, _dbl, _i64, _i32, _i32, _i32, _vp, _i32,
                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_sgpmc_mc_workspace_bytes": (_sz, [_i32, _i32]),
    "sgp_sgpmc_mc_tail": (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # ... with a composite kernel, a white-noise term and a mean function
    "sgp_sgpmc_comp_rows_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_sgpmc_comp_rows": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _dp, _dbl, _dbl, _vp, _i64, _i32, _i32, _i32, _vp, _i32,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_sgpmc_comp_bwd_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_sgpmc_comp_bwd": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _sz, _vp]),
    "sgp_suffstats_bwd_factored_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_suffstats_bwd_factored": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _vp, _vp, _dbl, _vp, _dbl, _i64, _i32, _i32, _i32,
                                          _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_suffstats_bwd_factored_workspace_bytes_ex": (_sz, [_i64, _i32, _i32, _i32]),
    "sgp_suffstats_bwd_factored_ex": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _vp, _vp, _dbl, _vp, _dbl, _i64, _i32, _i32, _i32,
                                             _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_set_cu_budget": (None, [_i32]),
    "sgp_small_supported": (_i32, [_i64, _i32, _i32, _i32]),
    "sgp_small_debug_stamps": (None, [_vp]),
    "sgp_small_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_small_sync_bytes": (_sz, []),
    "sgp_small_eval": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _dbl, _i32, _i32, _vp, _vp, _vp,
                              _vp, _sz, _vp]),
    "sgp_small_eval_composite": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _dp, _i32, _ip, _ip, _dp, _i64, _i32, _i32, _dbl, _i32, _i32,
                                        _vp, _vp, _vp, _sz, _vp]),
    "sgp_small_nuts_composite": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _dp, _i32, _ip, _ip, _dp, _i64, _i32, _i32, _dbl, _i32, _i32,
                                        _i32, _dbl, _dbl, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_small_eval_batch": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i32, _i64, _i32, _i32, _i32, _dbl, _i32, _i32, _vp, _vp, _vp, _vp,
                                    _vp, _sz, _vp]),
    "sgp_small_nuts_stat_cols": (_sz, []),
    "sgp_small_nuts": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _dbl, _i32, _i32, _i32, _dbl, _dbl,
                              C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_small_nuts_joint_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_small_nuts_joint": (_i32, [_vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _dbl, _i32, _i32, _i32, _dbl, _dbl, C.c_uint64,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_suffstats_bwd_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_suffstats_bwd": (_i32, [_vp, _i64, _vp, _vp, _i64, _dp, _dbl, _vp, _vp, _dbl, _vp, _i64, _i32, _i32, _i32,
                                 _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_kuu_bwd_workspace_bytes": (_sz, [_i32, _i32]),
    "sgp_kuu_bwd": (_i32, [_vp, _i64, _dp, _dbl, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_svgp_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_svgp_elbo": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _dp, _dbl, _dbl, _dbl, _vp, _vp, _i64, _i32, _i32, _i32, _i32,
                             _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_svgp_batch_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "sgp_svgp_elbo_batch": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _dp, _dp, _dp, _dbl, _vp, _vp, _i64, _i32, _i32, _i32, _i32,
                                   _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_svgp_elbo_batch_forward": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _dp, _dp, _dp, _dbl, _vp, _vp, _i64, _i32, _i32, _i32, _i32,
                                           _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_svgp_elbo_batch_reverse": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _dp, _dp, _dp, _dbl, _vp, _vp, _i64, _i32, _i32, _i32, _i32,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_svgp_predict_batch": (_i32, [_vp, _i64, _i64, _vp, _i64, _i32, _dp, _dp, _dbl, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_svgp_batch_combine": (_i32, [_i32, _dp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sgp_mixture_predict_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32, _i32, _i32]),
    "sgp_mixture_predict": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i32, _dp, _dp, _dp, _dbl, _i32, _i32, _i32, _i32, _dbl,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_mixture_predict_zs": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _dp, _dp, _dp, _dbl, _i32, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_svgp_predict": (_i32, [_vp, _i64, _i64, _vp, _i64, _dp, _dbl, _dbl, _vp, _vp, _i32, _i32, _i32,
                                _vp, _vp, _vp, _vp, _sz, _vp]),
    # the multi-class (robust-max) SVGP bound: C classes, m is C x M, LS is C x M x M
    "sgp_svgp_mc_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "sgp_svgp_mc_elbo": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _dp, _dbl, _dbl, _vp, _vp, _i32, _dbl, _i64, _i32, _i32, _i32, _i32,
                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_svgp_mc_predict": (_i32, [_vp, _i64, _i64, _vp, _i64, _dp, _dbl, _dbl, _vp, _vp, _i32, _dbl, _i32, _i32, _i32,
                                   _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_gauss_hermite": (_i32, [_i32, _dp, _dp]),
    # the exact GP marginal likelihood and its predictive (GPR_HMC)
    "sgp_exact_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_exact_factors_len": (_sz, [_i64]),
    "sgp_exact_eval": (_i32, [_vp, _i64, _vp, _i64, _i32, _dp, _dbl, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_exact_eval": (_i32, [_vp, _vp, _i64, _vp, _i64, _i32, _dp, _dbl, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_exact_predict_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "sgp_exact_predict": (_i32, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _dp, _dbl, _dbl, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_exact_predict": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _dp, _dbl, _dbl, _vp, _i32, _i32, _vp, _vp, _vp, _vp,
                                     _sz, _vp]),
    # P exact marginal likelihoods in one launch (LML surfaces, multi-start ML-II)
    "sgp_exact_batch_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "sgp_exact_batch_occupancy": (_i32, [_i32, _i32]),
    "sgp_exact_eval_batch": (_i32, [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgp_ctx_exact_eval_batch": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                        _sz, _vp]),
    "sgp_predict_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "sgp_predict": (_i32, [_vp, _i64, _i64, _vp, _i64, _dp, _dbl, _dbl, _vp, _i32, _i32, _i32, _i32,
                           _vp, _vp, _vp, _vp, _sz, _vp]),
}

# the companion library libsgp_exact_nuts_hip.so (include/sgp_exact_nuts.h): C device-resident NUTS chains over the exact marginal
# likelihood, one workgroup each (begin, then advance until all have finished)
EXACT_NUTS_LIB_PATH = os.path.join(HERE, "csrc", "libsgp_exact_nuts_hip.so")
EXACT_NUTS_PROTOTYPES = {
    "sgp_exact_nuts_batch_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "sgp_exact_nuts_batch_occupancy": (_i32, [_i32, _i32]),
    "sgp_exact_nuts_batch_begin": (_i32, _EN_BEGIN),
    "sgp_ctx_exact_nuts_batch_begin": (_i32, [_vp] + _EN_BEGIN),
    "sgp_exact_nuts_batch_advance": (_i32, _EN_ADVANCE),
    "sgp_ctx_exact_nuts_batch_advance": (_i32, [_vp] + _EN_ADVANCE),
}

# the companion library libsgp_exact_predict_hip.so (include/sgp_exact_predict.h): the exact-GP predictive of P problems in one launch
# and the mixture over the draws of a group
_EP_BATCH = [_vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]
EXACT_PREDICT_LIB_PATH = os.path.join(HERE, "csrc", "libsgp_exact_predict_hip.so")
EXACT_PREDICT_PROTOTYPES = {
    "sgp_exact_predict_batch_workspace_bytes": (_sz, [_i64, _i32, _i32, _i64]),
    "sgp_exact_predict_batch_occupancy": (_i32, [_i32, _i32]),
    "sgp_exact_predict_batch": (_i32, _EP_BATCH),
    "sgp_ctx_exact_predict_batch": (_i32, [_vp] + _EP_BATCH),
    "sgp_exact_mixture_workspace_bytes": (_sz, [_i64, _i64]),
    "sgp_exact_mixture_reduce": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# the companion library libsgp_vfe_batch_hip.so (include/sgp_vfe_batch.h): P collapsed sparse-GP bounds with their gradients in one launch
_VB_BATCH = [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _dbl, _i32, _vp, _vp, _vp, _vp,
             _sz, _vp]
VFE_BATCH_LIB_PATH = os.path.join(HERE, "csrc", "libsgp_vfe_batch_hip.so")
VFE_BATCH_PROTOTYPES = {
    "sgp_vfe_batch_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32, _i32]),
    "sgp_vfe_batch_occupancy": (_i32, [_i32, _i32]),
    "sgp_vfe_eval_batch": (_i32, _VB_BATCH),
    "sgp_ctx_vfe_eval_batch": (_i32, [_vp] + _VB_BATCH),
}
VFE_BATCH_MAX_M, VFE_BATCH_MAX_N, VFE_BATCH_MAX_D, VFE_BATCH_MAX_P = 64, 65536, 8, 2 ** 24 - 1  # the limits of sgp_vfe_eval_batch

# the companion library libsgp_vfe_nuts_hip.so (include/sgp_vfe_nuts.h): C device-resident NUTS chains over the collapsed bound at fixed
# inducing inputs, one workgroup each (begin, then advance until all have finished)
_VN_BEGIN = [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
_VN_ADVANCE = [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _vp,
               _i32, _vp, _vp, _sz, _vp]
VFE_NUTS_LIB_PATH = os.path.join(HERE, "csrc", "libsgp_vfe_nuts_hip.so")
VFE_NUTS_PROTOTYPES = {
    "sgp_vfe_nuts_batch_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "sgp_vfe_nuts_batch_occupancy": (_i32, [_i32, _i32]),
    "sgp_vfe_nuts_batch_begin": (_i32, _VN_BEGIN),
    "sgp_ctx_vfe_nuts_batch_begin": (_i32, [_vp] + _VN_BEGIN),
    "sgp_vfe_nuts_batch_advance": (_i32, _VN_ADVANCE),
    "sgp_ctx_vfe_nuts_batch_advance": (_i32, [_vp] + _VN_ADVANCE),
}
VFE_NUTS_BAD_START = 1  # SGP_VFE_NUTS_BAD_START

# the companion library libsgp_vfe_predict_hip.so (include/sgp_vfe_predict.h): the predictive of P collapsed sparse GPs in one launch
# (the mixture over the draws is sgp_exact_mixture_reduce of the exact predictive's library)
_VP_BATCH = [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _dbl,
             _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
VFE_PREDICT_LIB_PATH = os.path.join(HERE, "csrc", "libsgp_vfe_predict_hip.so")
VFE_PREDICT_PROTOTYPES = {
    "sgp_vfe_predict_batch_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i64]),
    "sgp_vfe_predict_batch_occupancy": (_i32, [_i32, _i32]),
    "sgp_vfe_predict_batch": (_i32, _VP_BATCH),
    "sgp_ctx_vfe_predict_batch": (_i32, [_vp] + _VP_BATCH),
}
VFE_PREDICT_MAX_T = 32768  # VP_MAXT

# the companion library libsgp_mixture_hip.so (include/sgp_mixture.h): quantiles and the PIT of the mixture over the draws of a group
_MQ = [_vp, _vp, _vp, _vp, _i64, _i64, _dp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
MIXTURE_LIB_PATH = os.path.join(HERE, "csrc", "libsgp_mixture_hip.so")
MIXTURE_PROTOTYPES = {
    "sgp_mixture_quantiles_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "sgp_mixture_quantiles": (_i32, _MQ),
    "sgp_ctx_mixture_quantiles": (_i32, [_vp] + _MQ),
}
MIXTURE_MAX_Q, MIXTURE_P_MIN = 8, 1e-9  # MQ_MAXQ, MQ_PMIN

# key -> (path, prototypes) of a companion library; _COMPANION_LIBS caches what has been loaded
_COMPANION_TABLE = {
    "exact_nuts": (EXACT_NUTS_LIB_PATH, EXACT_NUTS_PROTOTYPES),
    "exact_predict": (EXACT_PREDICT_LIB_PATH, EXACT_PREDICT_PROTOTYPES),
    "vfe_batch": (VFE_BATCH_LIB_PATH, VFE_BATCH_PROTOTYPES),
    "vfe_nuts": (VFE_NUTS_LIB_PATH, VFE_NUTS_PROTOTYPES),
    "vfe_predict": (VFE_PREDICT_LIB_PATH, VFE_PREDICT_PROTOTYPES),
    "mixture": (MIXTURE_LIB_PATH, MIXTURE_PROTOTYPES),
}
_LIB = None
_COMPANION_LIBS = {}


_BUILD_HINT = "Build it with `python -c 'import __graft_entry__ as g; g.build()'`"


def _bind(p: str, prototypes, missing: str):
    """dlopen ``p`` and bind every prototype; raises SgpLibraryError when anything is missing.  There is no fallback."""
    if not os.path.exists(p):
        raise SgpLibraryError("%s not found. %s%s" % (p, _BUILD_HINT, missing))
    try:
        lib = C.CDLL(p)
    except OSError as e:  # pragma: no cover - depends on the ROCm runtime being present
        raise SgpLibraryError("cannot load %s: %s" % (p, e)) from e
    for name, (res, args) in prototypes.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise SgpLibraryError("%s does not export %s" % (p, name)) from e
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path: str | None = None):
    """dlopen the HIP library and bind every prototype; raises SgpLibraryError when anything is missing."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    lib = _bind(path or LIB_PATH, PROTOTYPES, " (needs hipcc); this package has no CPU fallback.")
    if lib.sgp_abi_version() != SGP_ABI_VERSION:
        raise SgpLibraryError("ABI version mismatch: library %d, binding %d" % (lib.sgp_abi_version(), SGP_ABI_VERSION))
    if path is None:
        _LIB = lib
    return lib


def _load_companion(key):
    """dlopen a companion library (after the core library, which it links to) and bind its prototypes; no fallback either."""
    if key not in _COMPANION_LIBS:
        load_library()
        _COMPANION_LIBS[key] = _bind(*_COMPANION_TABLE[key], ".")
    return _COMPANION_LIBS[key]


def load_exact_nuts_library():
    """The batched sampler's library (include/sgp_exact_nuts.h)."""
    return _load_companion("exact_nuts")


def load_exact_predict_library():
    """The batched predictive's library (include/sgp_exact_predict.h)."""
    return _load_companion("exact_predict")


def load_vfe_batch_library():
    """The batched collapsed bound's library (include/sgp_vfe_batch.h)."""
    return _load_companion("vfe_batch")


def load_vfe_nuts_library():
    """The batched sparse sampler's library (include/sgp_vfe_nuts.h)."""
    return _load_companion("vfe_nuts")


def load_vfe_predict_library():
    """The batched sparse predictive's library (include/sgp_vfe_predict.h)."""
    return _load_companion("vfe_predict")


def load_mixture_library():
    """The mixture quantiles' library (include/sgp_mixture.h)."""
    return _load_companion("mixture")


def check(fn_name: str, status: int):
    if status != 0:
        lib = load_library()
        raise SgpStatusError(fn_name, status, lib.sgp_status_string(status).decode())
