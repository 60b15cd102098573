/* C ABI of libsgp_exact_predict_hip.so: the exact-GP predictive of P problems in one launch, and the mixture over the draws of a
 * group in a second one (csrc/sgp_exact_predict.hip).  A companion of libsgp_hip.so (include/sgp.h), which it links to and whose
 * types, status codes and contexts it uses; the core library's own surface (ABI version 3) is unchanged by it.
 *
 * sgp_exact_predict_batch.  Problem p is (data set X[ix[p]], target Y[iy[p]], test set Xs[ixs[p]], theta[p] = [ls_1..d | sf2 | s2]):
 *   A = sf2 k'(X, X; ls) + s2 I ; mean[p][t] = k*_t^T A^-1 y ; var[p][t] = sf2 - k*_t^T A^-1 k*_t (+ s2 with pred_noise != 0).
 * One workgroup per problem, the problem in its LDS: L = chol(A), L^-1 explicitly, alpha = L^-T L^-1 y, V = L^-1 K* on the fp64 matrix
 * cores, var = sf2 - sum_i V_it^2 -- the factorisation of sgp_exact_eval_batch without its gradient.
 *   X, Y, ix, iy: sgp_exact_eval_batch's convention (set s of X at X + s x_stride, row-major N x d with leading dimension ldx; ix / iy:
 *   P ints or NULL = set 0).  Xs: test set s at Xs + s xs_stride, T x d with leading dimension ldxs; ixs: P ints or NULL.
 *   1 <= N <= 128, 1 <= d <= 8, 1 <= T <= 32768, 1 <= P < 2^24, kernel_id 0..2 (SGP_KERNEL_COMPOSITE -> SGP_ERR_ARG); anything else
 *   is refused before anything is enqueued (SGP_ERR_ARG, then SGP_ERR_DIM, then SGP_ERR_WORKSPACE).  ws:
 *   sgp_exact_predict_batch_workspace_bytes(P, N, d, T) bytes (0 = unsupported shape).  Everything is DEVICE memory.
 *   Outputs: mean, var (P x T), info (P ints): 0, or the 1-based first pivot at which A is not numerically positive definite (the gate
 *   of sgp_exact_eval_batch: a pivot at or below 8 N 2^-53 (sf2 + s2); 1 for a row of theta that is not positive and finite).  A
 *   problem with info != 0 has NaN rows; its neighbours are untouched.  A failure is never an error return.
 *   The variance is NOT clamped, as in sgp_exact_predict: with pred_noise = 0 at a test point that coincides with a training point it
 *   is rounding noise around zero and may be negative.
 *   Determinism: no atomics; every sum has a fixed order that depends on N alone.  mean[p][t] and var[p][t] have the same bits for
 *   every T, P, stream, context and position in the batch.
 *   Accuracy (tests/exact_predict_reference.py, long double): with w = A^-1 k*, alpha = A^-1 y,
 *     |mean - ref| <= 1e-12 (|w|^T |A| |alpha| + |k*|^T |alpha|) ;  |var - ref| <= 1e-12 (|w|^T |A| |w| + 2 |k*|^T |w| + sf2)
 *   per test point -- first-order condition scales of the two quantities, with no factor cond(A).
 *
 * sgp_exact_mixture_reduce.  Problems [offsets[g], offsets[g + 1]) are the draws of group g (G groups, offsets: G + 1 int64, DEVICE,
 * non-decreasing from 0 to P -- the caller answers for that), all with T test points.  K = the draws with info == 0, n = |K|:
 *   mix_mean[g][t] = (1/n) sum mu_s ; mix_var[g][t] = (1/n) sum (v_s + (mu_s - mix_mean)^2)  (two passes) ; kept[g] = n ;
 *   with Ytest (G x T; NULL: logpdf / mean_logpdf are not written and may be NULL), l_s = log N(y_t | mu_s, v_s):
 *   logpdf[g][t] = log((1/n) sum exp l_s)  (max-shifted: the log of the mean density) ; mean_logpdf[g][t] = (1/n) sum l_s.
 *   n = 0: every output of the group is NaN.  A kept draw with v_s <= 0 makes the two density outputs NaN at that point.
 *   One thread per (g, t), serial over the draws in index order.  Rounding, against the same formulas evaluated exactly from the
 *   same mean / var (eps = 2^-53, q_s = (y - mu_s)^2 / (2 v_s), c_s = |log(2 pi v_s) / 2| + q_s):
 *     |d logpdf| <= eps (8 max c_s + n + 8) ; |d mean_logpdf| <= eps (8 + n) max c_s ;
 *     |d mix_mean| <= eps (n + 2) max |mu_s| ; |d mix_var| <= 2 eps (n + 4) max (v_s + (mu_s - mix_mean)^2).
 *   1 <= G < 2^24, 1 <= T <= 32768; ws: sgp_exact_mixture_workspace_bytes(G, T) bytes (0 = unsupported shape).
 * The sgp_ctx_* twin takes a context of libsgp_hip.so (NULL = the default one) and refuses one that belongs to another device
 * (SGP_ERR_ARG); neither kernel reads a context option, and the mixture has no twin.                                              */
#ifndef SGP_EXACT_PREDICT_H
#define SGP_EXACT_PREDICT_H
#include "sgp.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

size_t sgp_exact_predict_batch_workspace_bytes(int64_t P, int N, int d, int64_t T);
/* workgroups (= problems) of N's size class resident on one CU, from the runtime's occupancy query; < 0: a status (no launch) */
int sgp_exact_predict_batch_occupancy(int N, int kernel_id);
int sgp_exact_predict_batch(const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const double* Xs,
                            int64_t xs_stride, int64_t ldxs, int64_t T, const int* ix, const int* iy, const int* ixs, const double* theta,
                            int64_t P, int N, int d, int kernel_id, int pred_noise, double* mean, double* var, int* info, void* ws,
                            size_t ws_bytes, sgp_stream_t stream);
int sgp_ctx_exact_predict_batch(sgp_ctx* ctx, const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride,
                                const double* Xs, int64_t xs_stride, int64_t ldxs, int64_t T, const int* ix, const int* iy, const int* ixs,
                                const double* theta, int64_t P, int N, int d, int kernel_id, int pred_noise, double* mean, double* var,
                                int* info, void* ws, size_t ws_bytes, sgp_stream_t stream);
size_t sgp_exact_mixture_workspace_bytes(int64_t G, int64_t T);
int sgp_exact_mixture_reduce(const double* mean, const double* var, const int* info, const int64_t* offsets, int64_t G, int64_t T,
                             const double* Ytest, double* mix_mean, double* mix_var, double* logpdf, double* mean_logpdf, int* kept,
                             void* ws, size_t ws_bytes, sgp_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SGP_EXACT_PREDICT_H */
