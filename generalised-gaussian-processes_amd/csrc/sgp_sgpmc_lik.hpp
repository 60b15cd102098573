// Host-side launchers of the SGPMC row pass (sgp_sgpmc_lik.hip), shared with the composite-kernel row pass (sgp_sgpmc_comp.hip).
#pragma once
#include "sgp_common.hpp"

namespace sgp {

// Per datum of the Npad x Mp row-major T (Npad a multiple of ASM_ROWS): a_n = scale T_n, mu_n = a_n.v (+ mean_n), var_n = knn - |a_n|^2,
// the likelihood layer of sgp_lik.hpp with the floor 2^-40 knn, and out[SGP_SGPMC_LIK_OUT_LEN] = [sum ell | sum ds2 | sum dv] in a fixed
// order.  dmu_pad / dv_pad (Npad) are the zero-padded copies the adjoint launches read; part: 3 (Npad / ASM_ROWS) doubles; counter:
// one int the CALLER has cleared by a launch on `st` ahead of this one.  mean, mu_out, var_out may be null; y == nullptr: moments only
// (dmu, dv may be null as well).
void sgpmc_lik_rows_launch(const double* T, const double* y, const double* mean, const double* v, int64_t N, int64_t Npad, int M, int Mp,
                           double scale, double knn, double s2, int lik, double* dmu, double* dv, double* mu_out, double* var_out,
                           double* dmu_pad, double* dv_pad, double* part, int* counter, double* out, hipStream_t st);
// out <- 0: the same outputs for an empty shard
void sgpmc_lik_empty_launch(double* out, hipStream_t st);
// T_n <- sign sqrt(-dv_n) T_n in place, zeros in the padding
void sgpmc_lik_scale_launch(double* T, const double* dv_pad, int64_t N, int64_t Npad, int M, int Mp, double sign, hipStream_t st);

}  // namespace sgp
