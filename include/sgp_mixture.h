/* C ABI of libsgp_mixture_hip.so: quantiles and the probability integral transform (PIT) of the mixture over the draws of a group, in
 * one launch (csrc/sgp_mixture.hip; the arithmetic of one point is mq_point of csrc/sgp_mixture.hpp).  A companion of libsgp_hip.so
 * (include/sgp.h), which it links to and whose types, status codes and contexts it uses; the core library's own surface (ABI version
 * 3) is unchanged by it.
 *
 * sgp_mixture_quantiles.  mean, var (P x T), info (P ints), offsets (G + 1 int64), all DEVICE memory, are what
 * sgp_exact_mixture_reduce (include/sgp_exact_predict.h) takes: rows [offsets[g], offsets[g + 1]) are the draws of group g, offsets
 * non-decreasing from 0 to P -- the caller answers for that.  K = the draws of a group with info == 0, n = |K|, in index order; with
 * sigma_s = sqrt(v_s) and z_s = (x - mu_s) / sigma_s:
 *   lower tail G-(x) = (1/n) sum_s erfc(-z_s / sqrt 2) / 2 ;  upper tail G+(x) = (1/n) sum_s erfc(+z_s / sqrt 2) / 2.
 *   probs: Q probabilities on the HOST, 1 <= Q <= 8, each 1e-9 <= p <= 1 - 1e-9 (else SGP_ERR_ARG); they are copied into the launch
 *   arguments as (p_tail, side) = (p, lower) for p <= 1/2 and (1 - p, upper) above -- 1 - p is formed once, on the host.
 *   quant[g][q][t] (G x Q x T): the root of G-(x) = p_tail, or of G+(x) = p_tail on the upper side.
 *   pit[g][t] (G x T), with Ytest (G x T; NULL: pit is not written and may be NULL) = G-(y_t), one pass.
 *   iters[g][t] (G x T int32, or NULL): the passes over the draws the point took after its first, the largest count over the Q
 *   probabilities.
 *   n = 0: every output of the group is NaN.  A kept draw whose v is not positive and finite, or whose mu is not finite, makes every
 *   output NaN at that test point alone; neighbouring points and groups are untouched.  A failure is never an error return.
 * Accuracy contract.  The returned x is the midpoint of a final bracket [a, b] with
 *     b - a <= W(x) = 2^-48 (|x| + sigma_min),   sigma_min = the smallest kept sigma at that test point,
 *   where the kernel's own tail sum at a lies on the "quantile is above" side (G-(a) < p_tail, G+(a) > p_tail) and at b on the other.
 *   The bracket starts at [min_s (mu_s - z sigma_s), max_s (mu_s + z sigma_s)], z = sqrt(-2 ln p_tail), which contains the root
 *   (Phi(-z) <= p_tail / 2); both ends are verified with the kernel's tail sums and moved outwards if rounding broke them, and no
 *   iterate leaves the bracket.  Iterations: at most MQ_MAX_ITERS = 256 passes over the draws per point; a probability that has not
 *   met W by then is NaN (the bracket halves at least every fourth pass, and W is met
 *   after 48 + log2((hi - lo) / (|x| + sigma_min)) halvings; measured: 11 to 13 passes where the components' scales are
 *   alike, 41 to 68 with sigma from 1e-6 to 1e3 in one group, 60 at the median in the flat gap of a bimodal mixture).
 * Rounding of a tail sum, against the same formula evaluated exactly from the same mean / var:
 *     |tail_kernel(x) - tail_exact(x)| <= MQ_ERR(n, tail, sens) = 2^-52 ((n + c) tail + 2 sens),
 *     sens = (1/n) sum_s |z_s| phi(z_s)   (phi: the standard normal density),   c = MQ_C = 2 x 2.9902 + 4 = 9.9804.
 *   (n + 1) 2^-53 tail: the n serial additions and the division by n.  2 sens 2^-52: z_s / sqrt 2 is formed as (x - mu_s) times the
 *   rounded 1 / (sigma_s sqrt 2) -- six roundings (the subtraction, the square root, the reciprocal, the constant, two products),
 *   relative error <= 3 x 2^-53 < 2 x 2^-52, which moves a term Phi(z_s) by |z_s| phi(z_s) times that.
 *   c: the device erfc's error in ulps plus the scale by 1/2 and the slack above; the erfc's worst error measured on an MI355X against
 *   erfcl at 10^5 arguments in [-9, 9] is 2.9902 ulp (profiles/mixture_quantile_erfc_ulp.json), doubled because a sample does not
 *   bound a maximum.  pit: |pit - exact| <= (n + c) 2^-53, since |z| phi(z) <= 0.25 and pit <= 1.
 * Determinism: no atomics; one thread per (g, t), serial over the draws in index order, every sum from zero.  A (group, test point)
 *   has the same bits alone and at any position of any batch, for every Q and whatever the other probabilities are, on every launch,
 *   stream and context.
 * 1 <= G < 2^24, 1 <= T <= 32768 (else SGP_ERR_DIM); ws: sgp_mixture_quantiles_workspace_bytes(G, T, Q) bytes (0 = unsupported
 * shape), else SGP_ERR_WORKSPACE.  Refusals come before anything is enqueued: SGP_ERR_ARG, then SGP_ERR_DIM, then SGP_ERR_WORKSPACE.
 * The sgp_ctx_* twin takes a context of libsgp_hip.so (NULL = the default one) and refuses one that belongs to another device
 * (SGP_ERR_ARG); the kernel reads no context option.                                                                              */
#ifndef SGP_MIXTURE_H
#define SGP_MIXTURE_H
#include "sgp.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

size_t sgp_mixture_quantiles_workspace_bytes(int64_t G, int64_t T, int Q);
int sgp_mixture_quantiles(const double* mean, const double* var, const int* info, const int64_t* offsets, int64_t G, int64_t T,
                          const double* probs, int Q, const double* Ytest, double* quant, double* pit, int* iters, void* ws,
                          size_t ws_bytes, sgp_stream_t stream);
int sgp_ctx_mixture_quantiles(sgp_ctx* ctx, const double* mean, const double* var, const int* info, const int64_t* offsets, int64_t G,
                              int64_t T, const double* probs, int Q, const double* Ytest, double* quant, double* pit, int* iters,
                              void* ws, size_t ws_bytes, sgp_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SGP_MIXTURE_H */
