// P independent exact-GP marginal likelihoods in ONE launch (LML surfaces, multi-start ML-II): one 256-thread workgroup per problem, the
// whole problem in that workgroup's LDS (sgp_exact_batch.hpp: eb_load + eb_eval, shared with the batched NUTS of sgp_exact_nuts.hip).  No
// inter-workgroup communication, no flags, no spins, no atomics: a workgroup reads its data set and its row of theta, and writes its own
// rows of out / grads / info.  Every sum has a fixed order and depends on nothing outside the problem: the same bits on every call,
// stream and batch.
#include "sgp_exact_batch.hpp"

namespace sgp {

template <int KID, int NP>
__global__ __launch_bounds__(256) void exact_batch_kernel(const double* __restrict__ X, int64_t x_stride, int64_t ldx,
                                                          const double* __restrict__ Y, int64_t y_stride, const int* __restrict__ ix,
                                                          const int* __restrict__ iy, const double* __restrict__ theta, int N, int d,
                                                          int with_grad, double* __restrict__ out, double* __restrict__ grads,
                                                          int* __restrict__ info) {
  __shared__ EbShared<NP> sh;
  const int64_t p = blockIdx.x;
  const double* Xp = X + (int64_t)(ix ? ix[p] : 0) * x_stride;
  const double* Yp = Y + (int64_t)(iy ? iy[p] : 0) * y_stride;
  eb_load<NP>(sh, sh.yv, Xp, ldx, Yp, N, d);
  eb_eval<KID, NP>(sh, theta + p * (d + 2), N, d, with_grad, out + p * 4, grads + p * (d + 2), info + p);
}

}  // namespace sgp

using namespace sgp;

static int exact_batch_check(int64_t P, int N, int d, int kernel_id) {
  if (P <= 0 || N <= 0 || d <= 0) return SGP_ERR_ARG;
  if (kernel_id < 0 || kernel_id > SGP_KERNEL_MATERN52) return SGP_ERR_ARG;  // composite kernels: out of scope, as in sgp_exact_eval
  if (N > EB_MAXN || d > EB_MAXD || P > EB_MAXP) return SGP_ERR_DIM;
  return SGP_OK;
}

extern "C" size_t sgp_exact_batch_workspace_bytes(int64_t P, int N, int d, int with_grad) {
  (void)with_grad;
  return exact_batch_check(P, N, d, 0) == SGP_OK ? WG_WS_UNIT : 0;
}

// Workgroups of N's size class that one CU holds at a time, as the runtime counts them (registers and LDS of the loaded code object).
extern "C" int sgp_exact_batch_occupancy(int N, int kernel_id) {
  const int chk = exact_batch_check(1, N, 1, kernel_id);
  if (chk != SGP_OK) return chk;
  return with_kid_class<32, 64, 128>(kernel_id, eb_size_class(N),
                                     [](auto kid, auto np) { return wg_occupancy(exact_batch_kernel<kid(), np()>); });
}

extern "C" int sgp_exact_eval_batch(const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const int* ix,
                                    const int* iy, const double* theta, int64_t P, int N, int d, int kernel_id, int with_grad, double* out,
                                    double* grads, int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  const int chk = exact_batch_check(P, N, d, kernel_id);
  if (chk != SGP_OK) return chk;
  if (!X || !Y || !theta || !out || !info || (with_grad && !grads) || ldx < d || x_stride < 0 || y_stride < 0) return SGP_ERR_ARG;
  if (!ws || ws_bytes < sgp_exact_batch_workspace_bytes(P, N, d, with_grad)) return SGP_ERR_WORKSPACE;
  with_kid_class<32, 64, 128>(kernel_id, eb_size_class(N), [&](auto kid, auto np) {
    exact_batch_kernel<kid(), np()><<<dim3((unsigned)P), 256, 0, (hipStream_t)stream>>>(X, x_stride, ldx, Y, y_stride, ix, iy, theta, N, d,
                                                                                       with_grad ? 1 : 0, out, grads, info);
  });
  return check_launch();
}
