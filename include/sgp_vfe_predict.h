/* C ABI of libsgp_vfe_predict_hip.so: the predictive of P collapsed (Titsias / VFE) sparse GPs in one launch, one workgroup per
 * problem (csrc/sgp_vfe_predict.hip, csrc/sgp_vfe_predict.hpp).  A companion of libsgp_hip.so (include/sgp.h), which it links to and
 * whose types, status codes and contexts it uses; the core library's own surface (ABI version 3) is unchanged.
 *
 * Problem p is (data set X[ix[p]], target Y[iy[p]], inducing set Z[iz[p]], test set Xs[ixs[p]], theta[p] = [ls_1..d | sf2 | s2]), with
 * one jitter J for the call.  With sgp_vfe_batch.h's notation
 *   K = sf2 k'(Z, Z; ls) + J I ; L = chol K ; A = L^-1 K_uf ; B = I + A A^T / s2 ; L_B = chol B ; u = A y ; g = B^-1 u
 * the outputs are sgp_predict's predictive (include/sgp.h) per test point t, and the collapsed bound of the problem:
 *   a*_t = L^-1 k_u*(t) ; v_t = L_B^-1 a*_t ;
 *   mean[p][t] = a*_t^T g / s2 ;  var[p][t] = sf2 - sum_m a*_mt^2 + sum_m v_mt^2  (+ s2 with pred_noise != 0) ;
 *   bound[p] = F = logmarg - trace (P doubles, or NULL: not written), with the BITS of out[p][0] of sgp_vfe_eval_batch(want_grad = 0)
 *   on the same problem -- the training stage runs the same operations in the same order.
 *   The variance is NOT clamped, as in sgp_exact_predict_batch: it is ((sf2 - sum a*^2) + sum v^2) + s2 as the subtraction leaves it;
 *   with pred_noise = 0 and a tiny s2 it may be a small negative number at a test point that coincides with an inducing input.
 *   X, Y, Z, ix, iy, iz: sgp_vfe_eval_batch's convention (set s of X at X + s x_stride, row-major N x d with leading dimension ldx; Y:
 *   target s at Y + s y_stride; Z: set s at Z + s z_stride, M x d with leading dimension ldz; index arrays: P ints or NULL = set 0).
 *   Xs: test set s at Xs + s xs_stride, T x d with leading dimension ldxs; ixs: P ints or NULL.  Everything is DEVICE memory.
 *   1 <= M <= 64, 1 <= N <= 65536 (M > N is legal), 1 <= d <= 8, 1 <= T <= 32768, 1 <= P < 2^24, kernel_id 0..2
 *   (SGP_KERNEL_COMPOSITE -> SGP_ERR_ARG), J >= 0; anything else is refused before anything is enqueued (SGP_ERR_ARG, then
 *   SGP_ERR_DIM, then SGP_ERR_WORKSPACE).  ws: sgp_vfe_predict_batch_workspace_bytes(P, N, M, d, T) bytes (0 = unsupported shape); a
 *   placeholder as for sgp_vfe_eval_batch: the problem lives in its workgroup's LDS and the kernel neither reads nor writes ws.
 *   info (P ints): 0; k in 1..M: K is not numerically positive definite at pivot k (a pivot at or below 8 M 2^-53 (sf2 + J); 1 for a
 *   row of theta with an entry that is not a positive finite number); M + k: B is not positive definite at pivot k (a pivot at or below
 *   1/2).  A problem with info != 0 has NaN mean / var rows and a NaN bound; its neighbours are untouched.  A failure is never an error
 *   return.
 *   Determinism: no atomics, no inter-workgroup communication; every sum has a fixed order that depends on (N, M, d) alone -- the
 *   sums over m of a test point on M's size class alone.  mean[p][t], var[p][t] and bound[p] have the same bits for every T, P,
 *   position in the batch, stream and context.
 *   Accuracy (tests/vfe_predict_reference.py, long double): per test point, with the condition scales formed in the whitened basis
 *     S_mu = sum_m |a*_m| |g_m| / s2 ;  S_v = sf2 + sum a*^2 + sum v^2 (+ s2),
 *   |mean - ref| <= tol S_mu and |var - ref| <= tol S_v with tol = 10 max(e64, 1e-13), e64 the error of the float64 evaluation of
 *   the same closed form in the same units -- the rule sgp_vfe_eval_batch is held to.  There is no factor cond(K_uu).
 * The mixture over the draws of a group is sgp_exact_mixture_reduce (include/sgp_exact_predict.h) on these mean / var / info.
 * The sgp_ctx_* twin takes a context of libsgp_hip.so (NULL = the default one) and refuses one that belongs to another device
 * (SGP_ERR_ARG); the kernel reads no context option.                                                                              */
#ifndef SGP_VFE_PREDICT_H
#define SGP_VFE_PREDICT_H
#include "sgp.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

size_t sgp_vfe_predict_batch_workspace_bytes(int64_t P, int64_t N, int M, int d, int64_t T);
/* workgroups (= problems) of M's size class resident on one CU, from the runtime's occupancy query; < 0: a status (no launch) */
int sgp_vfe_predict_batch_occupancy(int M, int kernel_id);
int sgp_vfe_predict_batch(const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const int* ix, const int* iy,
                          const double* Z, int64_t z_stride, int64_t ldz, const int* iz, const double* Xs, int64_t xs_stride,
                          int64_t ldxs, int64_t T, const int* ixs, const double* theta, int64_t P, int64_t N, int M, int d, int kernel_id,
                          double jitter, int pred_noise, double* mean, double* var, double* bound, int* info, void* ws, size_t ws_bytes,
                          sgp_stream_t stream);
int sgp_ctx_vfe_predict_batch(sgp_ctx* ctx, const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride,
                              const int* ix, const int* iy, const double* Z, int64_t z_stride, int64_t ldz, const int* iz,
                              const double* Xs, int64_t xs_stride, int64_t ldxs, int64_t T, const int* ixs, const double* theta, int64_t P,
                              int64_t N, int M, int d, int kernel_id, double jitter, int pred_noise, double* mean, double* var,
                              double* bound, int* info, void* ws, size_t ws_bytes, sgp_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SGP_VFE_PREDICT_H */
