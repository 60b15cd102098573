/* C ABI of libsgp_vfe_nuts_hip.so: C independent NUTS chains over the collapsed (Titsias / VFE) sparse-GP bound at fixed inducing
 * inputs, device-resident (csrc/sgp_vfe_nuts.hip).  A companion of libsgp_hip.so (include/sgp.h), which it links to and whose types,
 * status codes and contexts it uses; the core library's own surface (ABI version 3) is unchanged by it.
 *
 * Chain c samples q = [log ls_1..d | log sig_f | log sig_n] of  F(X[ix[c]], Y[iy[c]], Z[iz[c]]; ls, sig_f^2, sig_n^2; jitter on K_uu)
 * + ls ~ Gamma(2, 1), sig_f, sig_n ~ HalfCauchy(1) + the log-Jacobians: the density of the Python HmcTarget, F the bound of
 * sgp_vfe_eval_batch (include/sgp_vfe_batch.h).  One workgroup per chain: thread 0 runs the sampler of sgp_small_nuts (same algorithm,
 * same splitmix64 stream from seed[c]), all 256 threads run the evaluation of sgp_vfe_eval_batch at the position it asks for.  Chains
 * share nothing (no cooperative launch, no spin).
 *   1 <= M <= 64, 1 <= N <= 65536 (M > N is legal), 1 <= d <= 8, 1 <= C < 2^24, kernel_id 0..2 (SGP_KERNEL_COMPOSITE -> SGP_ERR_ARG),
 *   jitter >= 0, 0 <= max_treedepth <= 11; anything else is refused before anything is enqueued (SGP_ERR_ARG, then SGP_ERR_DIM, then
 *   SGP_ERR_WORKSPACE).
 * sgp_vfe_nuts_batch_begin initialises the C chains in `ws` (sgp_vfe_nuts_batch_workspace_bytes(C, N, M, d) bytes, 0 = unsupported
 * shape; the per-chain sampler state and the evaluation's per-chain rows live there between launches) from q0 (DEVICE, C x (d + 2))
 * and seed (DEVICE, C).  sgp_vfe_nuts_batch_advance is ONE launch: every unfinished chain advances by at most evals_per_launch (>= 1)
 * evaluations, a finished chain exits at once; the call then reads back the number of finished chains into *finished (HOST; it
 * synchronises the stream).  The caller repeats it until *finished == C.  No output but `seconds` depends on evals_per_launch, bit for
 * bit.  X, Y, ix, iy, Z, iz: sgp_vfe_eval_batch's convention (ix / iy / iz: C ints or NULL).  Outputs (DEVICE), the same pointers in
 * every call:
 *   samples (C x n_draws x (d + 2)): post-tuning draws, unconstrained;  stats (C x n_draws x 8): sgp_small_nuts's columns
 *   [step_size, tree_size, depth, mean_tree_accept, diverging, energy, logp, cumulative evaluations];  seconds (C x n_draws): the
 *   device clock's time per draw;  evaluations, draws (C x int64), written when the chain finishes: evaluations consumed (the start's
 *   included), draws finished (tuning included);  info (C ints): 0, or SGP_VFE_NUTS_BAD_START -- the start has no finite density
 *   (an entry that is not finite or not inside +-300 included): that chain's samples / stats / seconds rows are NaN, its neighbours
 *   are untouched.  A failed factorisation during the run is a divergence (logp = -inf at that leaf), never an info.
 * The sgp_ctx_* twins take a context of libsgp_hip.so (NULL = the default one) and refuse one that belongs to another device
 * (SGP_ERR_ARG); the sampler reads no context option.                                                                          */
#ifndef SGP_VFE_NUTS_H
#define SGP_VFE_NUTS_H
#include "sgp.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define SGP_VFE_NUTS_BAD_START 1
size_t sgp_vfe_nuts_batch_workspace_bytes(int64_t C, int64_t N, int M, int d);
/* workgroups (= chains) of M's size class resident on one CU, from the runtime's occupancy query; < 0: a status (no launch) */
int sgp_vfe_nuts_batch_occupancy(int M, int kernel_id);
int sgp_vfe_nuts_batch_begin(const double* q0, const uint64_t* seed, int64_t C, int64_t N, int M, int d, int kernel_id, int n_tune,
                             int n_draws, int max_treedepth, double step_scale, double target_accept, double* samples, double* stats,
                             double* seconds, int64_t* evaluations, int64_t* draws, int* info, void* ws, size_t ws_bytes,
                             sgp_stream_t stream);
int sgp_vfe_nuts_batch_advance(const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const int* ix,
                               const int* iy, const double* Z, int64_t z_stride, int64_t ldz, const int* iz, int64_t C, int64_t N, int M,
                               int d, int kernel_id, double jitter, double* samples, double* stats, double* seconds,
                               int64_t* evaluations, int64_t* draws, int* info, int evals_per_launch, int64_t* finished, void* ws,
                               size_t ws_bytes, sgp_stream_t stream);
int sgp_ctx_vfe_nuts_batch_begin(sgp_ctx* ctx, const double* q0, const uint64_t* seed, int64_t C, int64_t N, int M, int d, int kernel_id,
                                 int n_tune, int n_draws, int max_treedepth, double step_scale, double target_accept, double* samples,
                                 double* stats, double* seconds, int64_t* evaluations, int64_t* draws, int* info, void* ws,
                                 size_t ws_bytes, sgp_stream_t stream);
int sgp_ctx_vfe_nuts_batch_advance(sgp_ctx* ctx, const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride,
                                   const int* ix, const int* iy, const double* Z, int64_t z_stride, int64_t ldz, const int* iz, int64_t C,
                                   int64_t N, int M, int d, int kernel_id, double jitter, double* samples, double* stats,
                                   double* seconds, int64_t* evaluations, int64_t* draws, int* info, int evals_per_launch,
                                   int64_t* finished, void* ws, size_t ws_bytes, sgp_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SGP_VFE_NUTS_H */
