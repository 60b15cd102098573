// The exact-GP predictive of P problems in ONE launch, and the mixture over the draws of a group in a second one
// (include/sgp_exact_predict.h).  Built into a library of its own, libsgp_exact_predict_hip.so, beside libsgp_hip.so: the core
// library's surface stays what it was.  The one thing taken from the core at link time is sgp_ctx_device, for the context twin.
//
// exact_predict_kernel: one 256-thread workgroup per problem (data set ix[p], target iy[p], test set ixs[p], theta[p]), the whole
// problem in that workgroup's LDS.  eb_load, eb_factor and eb_invert (sgp_exact_batch.hpp: the stages sgp_exact_eval_batch runs before
// its gradient) leave L^-1 in sh.M and alpha in sh.al; the kernel then walks the T test points in tiles of 16:
//   K*[k][t] = sf2 k'(x_k, xs_t) (zero for k >= N and for t >= T) ; mean[t] = sum_k K*[k][t] alpha[k] ;
//   V = L^-1 K* on the fp64 matrix cores, row tile i only over the column blocks k <= i (the zero blocks of L^-1 are never multiplied) ;
//   var[t] = sf2 - sum_i V[i][t]^2 (+ s2 with pred_noise), not clamped (sgp_exact_predict.hpp).
// V is never stored: a wave squares its accumulator tiles in registers, sums them down the rows, and leaves 16 partial sums in LDS; the
// four waves' words are added in a fixed order.
//
// The K* tile lies TRANSPOSED in LDS, ks[t][k] with the row stride NP + 2 of the image: in V = L^-1 K* it is the B operand, whose
// contraction index k then runs along a row -- the "16 rows x 4 consecutive columns" pattern of sgp_wg_dense.hpp, slots 2 t + c
// (mod 32) of a 32-lane group all distinct, the same as the A operand's read of L^-1.  Stored as k x 16 the operand would be "4 rows x
// 16 consecutive columns", which no stride below 32 separates without permuting the rows of a 16-block (stride 17: one 2-way conflict
// per read; the image's row permutation needs 16 slots between rows 8 apart, which 17 does not give).  The transposed tile is also the
// smaller one (16 x 130 against 128 x 17 doubles), its assembly writes and the mean's reads run along rows.
//
// Row tiles to waves: wave w takes tile w and, past the fourth tile, tile nb - 1 - w (cost i + 1 blocks for tile i: the pairs balance).
// The assignment, and with it every sum's order, depends on N alone: a test point's mean / var do not depend on T, on P, on the
// stream or on the grid.  No atomics, no flags, no spins, no inter-workgroup communication.
//
// exact_mixture_kernel: one thread per (group, test point), serial over the group's draws in index order (ep_mix_point,
// sgp_exact_predict.hpp); neighbouring threads read neighbouring test points of a draw's row.
#include "../../include/sgp_exact_predict.h"
#include "sgp_exact_batch.hpp"
#include "sgp_exact_predict.hpp"

namespace sgp {

template <int NP>
struct EpShared {
  EbShared<NP> eb;
  double ks[EP_TILE][NP + 2];   // K* tile, transposed: ks[t][k]
  double xs[EP_TILE][EB_XLD];   // the tile's test points
  double part[4][EP_TILE];      // the waves' partial sums of V^2 down the rows
};
static_assert(sizeof(EpShared<128>) <= 160 * 1024, "the large class must fit the CU's LDS");

struct EpArgs {
  const double *X, *Y, *Xs, *theta;
  int64_t x_stride, ldx, y_stride, xs_stride, ldxs;
  const int *ix, *iy, *ixs;
  int T, N, d, pred_noise;
  double *mean, *var;
  int* info;
};

template <int KID, int NP>
__global__ __launch_bounds__(256) void exact_predict_kernel(EpArgs a) {
  __shared__ EpShared<NP> es;
  EbShared<NP>& sh = es.eb;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int N = a.N, d = a.d, T = a.T;
  const int Nr = round_up(N, 16), nb = Nr / 16;
  const int64_t p = blockIdx.x;
  const double* Xp = a.X + (int64_t)(a.ix ? a.ix[p] : 0) * a.x_stride;
  const double* Yp = a.Y + (int64_t)(a.iy ? a.iy[p] : 0) * a.y_stride;
  const double* Xsp = a.Xs + (int64_t)(a.ixs ? a.ixs[p] : 0) * a.xs_stride;
  const double* th = a.theta + p * (d + 2);
  double* mean = a.mean + p * (int64_t)T;
  double* var = a.var + p * (int64_t)T;

  eb_load<NP>(sh, sh.yv, Xp, a.ldx, Yp, N, d);
  double ils[EB_MAXD];
  const EbValue val = eb_factor<KID, NP>(sh, th, N, d, ils);
  if (val.bad != 0) {  // (uniform over the workgroup)
    const double nan = __builtin_nan("");
    for (int t = tid; t < T; t += 256) {
      mean[t] = nan;
      var[t] = nan;
    }
    if (tid == 0) a.info[p] = val.bad;
    return;
  }
  eb_invert<NP>(sh, N);  // (ends on a barrier: sh.M = L^-1, sh.al = alpha)
  const double sf2 = th[d], s2 = th[d + 1];
  const double noise = a.pred_noise ? s2 : 0.0;

  for (int t0 = 0; t0 < T; t0 += EP_TILE) {
    for (int e = tid; e < EP_TILE * d; e += 256) {
      const int t = e / d, q = e - t * d;
      es.xs[t][q] = t0 + t < T ? Xsp[(int64_t)(t0 + t) * a.ldxs + q] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < EP_TILE * Nr; e += 256) {
      const int t = e / Nr, k = e - t * Nr;
      double v = 0.0;
      if (k < N && t0 + t < T) {
        double r2 = 0.0;
#pragma unroll
        for (int q = 0; q < EB_MAXD; ++q) {
          if (q < d) {
            const double df = (sh.x[k][q] - es.xs[t][q]) * ils[q];
            r2 = fma(df, df, r2);
          }
        }
        v = sf2 * kprofile<KID>(r2);
      }
      es.ks[t][k] = v;
    }
    __syncthreads();
    {  // mean: 16 threads per test point, thread j the entries j, j + 16, ..., then the 16 partial sums by a fixed butterfly
      const int t = tid >> 4, j = tid & 15;
      double s = 0.0;
      for (int k = j; k < Nr; k += 16) s = fma(es.ks[t][k], sh.al[k], s);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (j == 0 && t0 + t < T) mean[t0 + t] = s;
    }
    double sq = 0.0;  // this lane's share of sum_i V[i][t]^2, t = l15
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = u == 0 ? wave : nb - 1 - wave;
      if (u == 0 ? i < nb : i > 3) {
        const int i0 = 16 * i;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 <= i0; k0 += 16) {
#pragma unroll
          for (int s = 0; s < 4; ++s) acc = mfma16(sh.M[i0 + l15][k0 + 4 * s + l4], es.ks[l15][k0 + 4 * s + l4], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sq = fma(acc[r], acc[r], sq);
      }
    }
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);
    if (lane < 16) es.part[wave][l15] = sq;
    __syncthreads();
    if (tid < EP_TILE && t0 + tid < T)  // sgp_exact_predict's order: (sf2 - sum) + s2
      var[t0 + tid] = sf2 - ((es.part[0][tid] + es.part[1][tid]) + (es.part[2][tid] + es.part[3][tid])) + noise;
  }
  if (tid == 0) a.info[p] = 0;
}

// Work item = (group, chunk of 256 test points); the items are dealt to the workgroups in a fixed stride.  Nothing is summed across
// threads, so how the items are dealt changes no bit.
__global__ __launch_bounds__(256) void exact_mixture_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                            const int* __restrict__ info, const long long* __restrict__ offsets,
                                                            long long G, int T, const double* __restrict__ Ytest,
                                                            double* __restrict__ mix_mean, double* __restrict__ mix_var,
                                                            double* __restrict__ logpdf, double* __restrict__ mean_logpdf,
                                                            int* __restrict__ kept) {
  const long long chunks = (T + 255) / 256;
  for (long long item = blockIdx.x; item < G * chunks; item += gridDim.x) {
    const long long g = item / chunks;
    const int t = (int)(item - g * chunks) * 256 + (int)threadIdx.x;
    if (t >= T) continue;
    const long long s0 = offsets[g], s1 = offsets[g + 1];
    const EpMixPoint r = ep_mix_point(mean + s0 * T + t, var + s0 * T + t, info + s0, s1 - s0, T, Ytest != nullptr,
                                      Ytest ? Ytest[g * T + t] : 0.0);
    mix_mean[g * T + t] = r.mean;
    mix_var[g * T + t] = r.var;
    if (Ytest) {
      logpdf[g * T + t] = r.logpdf;
      mean_logpdf[g * T + t] = r.mean_logpdf;
    }
    if (t == 0) kept[g] = (int)r.kept;
  }
}

}  // namespace sgp

using namespace sgp;

static int exact_predict_check(int64_t P, int N, int d, int64_t T, int kernel_id) {
  if (P <= 0 || N <= 0 || d <= 0 || T <= 0) return SGP_ERR_ARG;
  if (kernel_id < 0 || kernel_id > SGP_KERNEL_MATERN52) return SGP_ERR_ARG;  // composite kernels: out of scope, as in sgp_exact_eval_batch
  if (N > EB_MAXN || d > EB_MAXD || P > EB_MAXP || T > EP_MAXT) return SGP_ERR_DIM;
  return SGP_OK;
}

extern "C" size_t sgp_exact_predict_batch_workspace_bytes(int64_t P, int N, int d, int64_t T) {
  return exact_predict_check(P, N, d, T, 0) == SGP_OK ? WG_WS_UNIT : 0;
}

// Workgroups of N's size class that one CU holds at a time, as the runtime counts them (registers and LDS of the loaded code object).
extern "C" int sgp_exact_predict_batch_occupancy(int N, int kernel_id) {
  const int chk = exact_predict_check(1, N, 1, 1, kernel_id);
  if (chk != SGP_OK) return chk;
  return with_kid_class<32, 64, 128>(kernel_id, eb_size_class(N),
                                     [](auto kid, auto np) { return wg_occupancy(exact_predict_kernel<kid(), np()>); });
}

extern "C" int sgp_exact_predict_batch(const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const double* Xs,
                                       int64_t xs_stride, int64_t ldxs, int64_t T, const int* ix, const int* iy, const int* ixs,
                                       const double* theta, int64_t P, int N, int d, int kernel_id, int pred_noise, double* mean,
                                       double* var, int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  const int chk = exact_predict_check(P, N, d, T, kernel_id);
  if (chk != SGP_OK && chk != SGP_ERR_DIM) return chk;
  if (!X || !Y || !Xs || !theta || !mean || !var || !info || ldx < d || ldxs < d || x_stride < 0 || y_stride < 0 || xs_stride < 0)
    return SGP_ERR_ARG;
  if (chk != SGP_OK) return chk;
  if (!ws || ws_bytes < sgp_exact_predict_batch_workspace_bytes(P, N, d, T)) return SGP_ERR_WORKSPACE;
  EpArgs a{};
  a.X = X, a.Y = Y, a.Xs = Xs, a.theta = theta;
  a.x_stride = x_stride, a.ldx = ldx, a.y_stride = y_stride, a.xs_stride = xs_stride, a.ldxs = ldxs;
  a.ix = ix, a.iy = iy, a.ixs = ixs;
  a.T = (int)T, a.N = N, a.d = d, a.pred_noise = pred_noise ? 1 : 0;
  a.mean = mean, a.var = var, a.info = info;
  with_kid_class<32, 64, 128>(kernel_id, eb_size_class(N), [&](auto kid, auto np) {
    exact_predict_kernel<kid(), np()><<<dim3((unsigned)P), 256, 0, (hipStream_t)stream>>>(a);
  });
  return check_launch();
}

extern "C" int sgp_ctx_exact_predict_batch(sgp_ctx* ctx, const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride,
                                           const double* Xs, int64_t xs_stride, int64_t ldxs, int64_t T, const int* ix, const int* iy,
                                           const int* ixs, const double* theta, int64_t P, int N, int d, int kernel_id, int pred_noise,
                                           double* mean, double* var, int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!ctx_device_matches(ctx)) return SGP_ERR_ARG;
  return sgp_exact_predict_batch(X, x_stride, ldx, Y, y_stride, Xs, xs_stride, ldxs, T, ix, iy, ixs, theta, P, N, d, kernel_id, pred_noise,
                                 mean, var, info, ws, ws_bytes, stream);
}

static int exact_mixture_check(int64_t G, int64_t T) {
  if (G <= 0 || T <= 0) return SGP_ERR_ARG;
  if (G > EB_MAXP || T > EP_MAXT) return SGP_ERR_DIM;
  return SGP_OK;
}

extern "C" size_t sgp_exact_mixture_workspace_bytes(int64_t G, int64_t T) { return exact_mixture_check(G, T) == SGP_OK ? WG_WS_UNIT : 0; }

extern "C" int sgp_exact_mixture_reduce(const double* mean, const double* var, const int* info, const int64_t* offsets, int64_t G, int64_t T,
                                        const double* Ytest, double* mix_mean, double* mix_var, double* logpdf, double* mean_logpdf,
                                        int* kept, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  const int chk = exact_mixture_check(G, T);
  if (chk != SGP_OK && chk != SGP_ERR_DIM) return chk;
  if (!mean || !var || !info || !offsets || !mix_mean || !mix_var || !kept || (Ytest && (!logpdf || !mean_logpdf))) return SGP_ERR_ARG;
  if (chk != SGP_OK) return chk;
  if (!ws || ws_bytes < sgp_exact_mixture_workspace_bytes(G, T)) return SGP_ERR_WORKSPACE;
  const int64_t items = G * ((T + 255) / 256);
  const unsigned grid = (unsigned)(items < (1 << 20) ? items : (1 << 20));
  exact_mixture_kernel<<<dim3(grid), 256, 0, (hipStream_t)stream>>>(mean, var, info, reinterpret_cast<const long long*>(offsets), G, (int)T,
                                                                    Ytest, mix_mean, mix_var, logpdf, mean_logpdf, kept);
  return check_launch();
}
