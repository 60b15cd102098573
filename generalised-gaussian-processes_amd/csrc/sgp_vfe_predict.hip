// The predictive of P collapsed (Titsias / VFE) sparse GPs in ONE launch, one 256-thread workgroup per problem
// (include/sgp_vfe_predict.h; the evaluation itself is vp_eval of sgp_vfe_predict.hpp).  Built into a library of its own,
// libsgp_vfe_predict_hip.so, beside libsgp_hip.so: the core library's surface stays what it was.  The one thing taken from the core at
// link time is sgp_ctx_device, for the context twin.  The mixture over the draws of a group is sgp_exact_mixture_reduce
// (libsgp_exact_predict_hip.so), which works on any mean / var / info / offsets: it is not rebuilt here.
#include "../../include/sgp_vfe_predict.h"
#include "sgp_vfe_predict.hpp"

namespace sgp {

// vfe_batch_kernel's register bounds (sgp_vfe_batch.hip): the small and the middle class are held to 256 registers, so that a CU takes
// two of their workgroups (their LDS, VbShared<MP> and nothing else, allows it); the large class fills the LDS of a CU alone.
template <int KID, int MP>
__global__ __launch_bounds__(256, MP == 64 ? 1 : 2) void vfe_predict_kernel(VpArgs a) {
  __shared__ VbShared<MP> sh;
  vp_eval<KID, MP>(sh, a, (int64_t)blockIdx.x);
}

}  // namespace sgp

using namespace sgp;

extern "C" size_t sgp_vfe_predict_batch_workspace_bytes(int64_t P, int64_t N, int M, int d, int64_t T) {
  return vp_workspace_bytes(P, N, M, d, T);
}

// Workgroups of M's size class that one CU holds at a time, as the runtime counts them (registers and LDS of the loaded code object).
extern "C" int sgp_vfe_predict_batch_occupancy(int M, int kernel_id) {
  const int chk = vp_check(1, 1, M, 1, 1, kernel_id);
  if (chk != SGP_OK) return chk;
  return with_kid_class<16, 32, 64>(kernel_id, vb_size_class(M),
                                    [](auto kid, auto mp) { return wg_occupancy(vfe_predict_kernel<kid(), mp()>); });
}

extern "C" int sgp_vfe_predict_batch(const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const int* ix,
                                     const int* iy, const double* Z, int64_t z_stride, int64_t ldz, const int* iz, const double* Xs,
                                     int64_t xs_stride, int64_t ldxs, int64_t T, const int* ixs, const double* theta, int64_t P, int64_t N,
                                     int M, int d, int kernel_id, double jitter, int pred_noise, double* mean, double* var, double* bound,
                                     int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  const int chk = vp_check(P, N, M, d, T, kernel_id);
  if (chk != SGP_OK && chk != SGP_ERR_DIM) return chk;
  if (!X || !Y || !Z || !Xs || !theta || !mean || !var || !info || ldx < d || ldz < d || ldxs < d || x_stride < 0 || y_stride < 0 ||
      z_stride < 0 || xs_stride < 0 || !(jitter >= 0.0))
    return SGP_ERR_ARG;
  if (chk != SGP_OK) return chk;
  if (!ws || ws_bytes < vp_workspace_bytes(P, N, M, d, T)) return SGP_ERR_WORKSPACE;
  VpArgs a{};
  a.X = X, a.Y = Y, a.Z = Z, a.Xs = Xs, a.theta = theta;
  a.x_stride = x_stride, a.ldx = ldx, a.y_stride = y_stride, a.z_stride = z_stride, a.ldz = ldz, a.xs_stride = xs_stride, a.ldxs = ldxs;
  a.ix = ix, a.iy = iy, a.iz = iz, a.ixs = ixs;
  a.N = (int)N, a.M = M, a.d = d, a.T = (int)T, a.pred_noise = pred_noise ? 1 : 0;
  a.jitter = jitter;
  a.mean = mean, a.var = var, a.bound = bound, a.info = info;
  with_kid_class<16, 32, 64>(kernel_id, vb_size_class(M), [&](auto kid, auto mp) {
    vfe_predict_kernel<kid(), mp()><<<dim3((unsigned)P), 256, 0, (hipStream_t)stream>>>(a);
  });
  return check_launch();
}

extern "C" int sgp_ctx_vfe_predict_batch(sgp_ctx* ctx, const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride,
                                         const int* ix, const int* iy, const double* Z, int64_t z_stride, int64_t ldz, const int* iz,
                                         const double* Xs, int64_t xs_stride, int64_t ldxs, int64_t T, const int* ixs, const double* theta,
                                         int64_t P, int64_t N, int M, int d, int kernel_id, double jitter, int pred_noise, double* mean,
                                         double* var, double* bound, int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!ctx_device_matches(ctx)) return SGP_ERR_ARG;
  return sgp_vfe_predict_batch(X, x_stride, ldx, Y, y_stride, ix, iy, Z, z_stride, ldz, iz, Xs, xs_stride, ldxs, T, ixs, theta, P, N, M, d,
                               kernel_id, jitter, pred_noise, mean, var, bound, info, ws, ws_bytes, stream);
}
