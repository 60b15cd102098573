// Quantiles and the PIT of the mixture over the draws of a group, on the moments sgp_exact_mixture_reduce takes (include/sgp_mixture.h;
// the arithmetic of a point is mq_point of sgp_mixture.hpp).  Built into a library of its own, libsgp_mixture_hip.so, beside
// libsgp_hip.so: the core library's surface stays what it was.  The one thing taken from the core at link time is sgp_ctx_device, for
// the context twin.
//
// mixture_quantile_kernel: one thread per (group, test point), serial over the group's draws in index order, as exact_mixture_kernel
// (sgp_exact_predict.hip): neighbouring threads read neighbouring test points of a draw's row, nothing is summed across threads, so how
// the items are dealt to the workgroups changes no bit.  The points of a wave take different numbers of passes; a lane that has
// finished waits for the slowest of its 64 (DESIGN 6e-9 has the measured spread).  NQ, the compile-time size of the per-probability
// state, is the smallest of 1, 2, 4, 8 that holds Q: the state stays in registers, and a probability's arithmetic does not depend on it.
#include "../../include/sgp_mixture.h"
#include "sgp_exact_batch.hpp"
#include "sgp_exact_predict.hpp"
#include "sgp_mixture.hpp"
#include "sgp_wg_dense.hpp"

namespace sgp {

static_assert(MQ_MAXG == EB_MAXP && MQ_MAXT == EP_MAXT, "the limits of the sibling mixture kernel");

template <int NQ>
__global__ __launch_bounds__(256) void mixture_quantile_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                               const int* __restrict__ info, const long long* __restrict__ offsets,
                                                               long long G, int T, MqProbs pr, int Q, const double* __restrict__ Ytest,
                                                               double* __restrict__ quant, double* __restrict__ pit,
                                                               int* __restrict__ iters) {
  const long long chunks = (T + 255) / 256;
  for (long long item = blockIdx.x; item < G * chunks; item += gridDim.x) {
    const long long g = item / chunks;
    const int t = (int)(item - g * chunks) * 256 + (int)threadIdx.x;
    if (t >= T) continue;
    const long long s0 = offsets[g], s1 = offsets[g + 1];
    double qv[NQ], pv;
    int itv;
    mq_point<NQ>(mean + s0 * T + t, var + s0 * T + t, info + s0, s1 - s0, T, Q, pr, Ytest != nullptr, Ytest ? Ytest[g * T + t] : 0.0, qv,
                 &pv, &itv);
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (q < Q) quant[(g * Q + q) * T + t] = qv[q];
    if (Ytest) pit[g * T + t] = pv;
    if (iters) iters[g * T + t] = itv;
  }
}

}  // namespace sgp

using namespace sgp;

static int mixture_quantiles_check(int64_t G, int64_t T, int Q) {
  if (G <= 0 || T <= 0 || Q <= 0 || Q > MQ_MAXQ) return SGP_ERR_ARG;
  if (G > MQ_MAXG || T > MQ_MAXT) return SGP_ERR_DIM;
  return SGP_OK;
}

extern "C" size_t sgp_mixture_quantiles_workspace_bytes(int64_t G, int64_t T, int Q) {
  return mixture_quantiles_check(G, T, Q) == SGP_OK ? WG_WS_UNIT : 0;
}

extern "C" int sgp_mixture_quantiles(const double* mean, const double* var, const int* info, const int64_t* offsets, int64_t G, int64_t T,
                                     const double* probs, int Q, const double* Ytest, double* quant, double* pit, int* iters, void* ws,
                                     size_t ws_bytes, sgp_stream_t stream) {
  const int chk = mixture_quantiles_check(G, T, Q);
  if (chk != SGP_OK && chk != SGP_ERR_DIM) return chk;
  if (!mean || !var || !info || !offsets || !probs || !quant || (Ytest && !pit)) return SGP_ERR_ARG;
  MqProbs pr{};
  for (int q = 0; q < Q; ++q) {
    if (!mq_prob_ok(probs[q])) return SGP_ERR_ARG;
    mq_split(probs[q], &pr.p_tail[q], &pr.upper[q]);
  }
  for (int q = Q; q < MQ_MAXQ; ++q) pr.p_tail[q] = 0.5;  // never read by a thread's results; keeps pass 0 finite
  if (chk != SGP_OK) return chk;
  if (!ws || ws_bytes < sgp_mixture_quantiles_workspace_bytes(G, T, Q)) return SGP_ERR_WORKSPACE;
  const int64_t items = G * ((T + 255) / 256);
  const dim3 grid((unsigned)(items < (1 << 20) ? items : (1 << 20)));
  const long long* off = reinterpret_cast<const long long*>(offsets);
  hipStream_t st = (hipStream_t)stream;
  if (Q == 1)
    mixture_quantile_kernel<1><<<grid, 256, 0, st>>>(mean, var, info, off, G, (int)T, pr, Q, Ytest, quant, pit, iters);
  else if (Q == 2)
    mixture_quantile_kernel<2><<<grid, 256, 0, st>>>(mean, var, info, off, G, (int)T, pr, Q, Ytest, quant, pit, iters);
  else if (Q <= 4)
    mixture_quantile_kernel<4><<<grid, 256, 0, st>>>(mean, var, info, off, G, (int)T, pr, Q, Ytest, quant, pit, iters);
  else
    mixture_quantile_kernel<8><<<grid, 256, 0, st>>>(mean, var, info, off, G, (int)T, pr, Q, Ytest, quant, pit, iters);
  return check_launch();
}

extern "C" int sgp_ctx_mixture_quantiles(sgp_ctx* ctx, const double* mean, const double* var, const int* info, const int64_t* offsets,
                                         int64_t G, int64_t T, const double* probs, int Q, const double* Ytest, double* quant, double* pit,
                                         int* iters, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!ctx_device_matches(ctx)) return SGP_ERR_ARG;
  return sgp_mixture_quantiles(mean, var, info, offsets, G, T, probs, Q, Ytest, quant, pit, iters, ws, ws_bytes, stream);
}
