/* C ABI of libsgp_vfe_batch_hip.so: P independent collapsed (Titsias / VFE) sparse-GP bounds with their complete gradients in one
 * launch, one workgroup per problem (csrc/sgp_vfe_batch.hip, csrc/sgp_vfe_batch.hpp).  A companion of libsgp_hip.so (include/sgp.h),
 * which it links to and whose types, status codes and contexts it uses; the core library's own surface (ABI version 3) is unchanged.
 *
 * Problem p is (data set X[ix[p]], target Y[iy[p]], inducing set Z[iz[p]], theta[p] = [ls_1..d | sf2 | s2]), with one jitter J for the
 * call:
 *   K = sf2 k'(Z, Z; ls) + J I ; L = chol K ; A = L^-1 K_uf ; B = I + A A^T / s2 ; F = logmarg - trace, the bound of sgp_small_eval
 *   (mode 0), with dF/dls, dF/dsf2, dF/ds2 and, on request, dF/dZ.
 *   X: set s at X + s x_stride, row-major N x d with leading dimension ldx; Y: target s at Y + s y_stride (N doubles); Z: set s at
 *   Z + s z_stride, M x d with leading dimension ldz; ix / iy / iz: P ints or NULL = set 0 for every problem.  Everything is DEVICE
 *   memory.
 *   1 <= M <= 64, 1 <= N <= 65536 (M > N is legal), 1 <= d <= 8, 1 <= P < 2^24, kernel_id 0..2 (SGP_KERNEL_COMPOSITE -> SGP_ERR_ARG),
 *   J >= 0; anything else is refused before anything is enqueued (SGP_ERR_ARG, then SGP_ERR_DIM, then SGP_ERR_WORKSPACE).
 *   ws: sgp_vfe_batch_workspace_bytes(P, N, M, d, want_grad, want_gz) bytes (0 = unsupported shape).
 *   The workspace is a placeholder: a problem lives in its workgroup's LDS and the kernel neither reads nor writes ws.  The query and
 *   the non-NULL buffer keep the convention of the library's other entry points, so that a later size class with an image in global
 *   scratch can use it without a change of this ABI.
 *   Outputs: out (P x (d + 5)), sgp_small_eval's natural layout [F | dF/dls_1..d | dF/dsf2 | dF/ds2 | logmarg | trace]; want_grad = 0
 *   writes F, logmarg and trace and NaN in the gradient slots, F with the same bits as with gradients.  g_Z (P x M x d, or NULL).
 *   info (P ints): 0; k in 1..M: K is not numerically positive definite at pivot k (a pivot at or below 8 M 2^-53 (sf2 + J); 1 for a
 *   row of theta with an entry that is not a positive finite number); M + k: B is not positive definite at pivot k (a pivot at or below
 *   1/2, where exact arithmetic gives at least 1).  A problem with info != 0 has NaN rows; its neighbours are untouched.  A failure is
 *   never an error return.
 *   Determinism: no atomics, no inter-workgroup communication; every sum has a fixed order that depends on (N, M, d) alone.  A
 *   problem's outputs have the same bits for every P, position in the batch, stream and context.
 *   Accuracy (tests/vfe_reference.py, long double): every output component-wise within 10 max(e64, 1e-13) of the reference in units
 *   of its condition scale (the same sum with every final factor in absolute value, formed in the whitened basis), e64 the error of
 *   the float64 evaluation of the same closed form -- the statement sgp_small_eval is held to.  There is no factor cond(K_uu): the
 *   adjoints are applied to A_t = L^-1 K_uf,t in the whitened basis, never as an unwhitened M x M matrix to K_uf.
 * The sgp_ctx_* twin takes a context of libsgp_hip.so (NULL = the default one) and refuses one that belongs to another device
 * (SGP_ERR_ARG); the kernel reads no context option.                                                                              */
#ifndef SGP_VFE_BATCH_H
#define SGP_VFE_BATCH_H
#include "sgp.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

size_t sgp_vfe_batch_workspace_bytes(int64_t P, int64_t N, int M, int d, int want_grad, int want_gz);
/* workgroups (= problems) of M's size class resident on one CU, from the runtime's occupancy query; < 0: a status (no launch) */
int sgp_vfe_batch_occupancy(int M, int kernel_id);
int sgp_vfe_eval_batch(const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const int* ix, const int* iy,
                       const double* Z, int64_t z_stride, int64_t ldz, const int* iz, const double* theta, int64_t P, int64_t N, int M,
                       int d, int kernel_id, double jitter, int want_grad, double* out, double* g_Z, int* info, void* ws, size_t ws_bytes,
                       sgp_stream_t stream);
int sgp_ctx_vfe_eval_batch(sgp_ctx* ctx, const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const int* ix,
                           const int* iy, const double* Z, int64_t z_stride, int64_t ldz, const int* iz, const double* theta, int64_t P,
                           int64_t N, int M, int d, int kernel_id, double jitter, int want_grad, double* out, double* g_Z, int* info,
                           void* ws, size_t ws_bytes, sgp_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SGP_VFE_BATCH_H */
