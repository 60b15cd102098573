// P independent collapsed (Titsias / VFE) sparse-GP bounds with their complete gradients in ONE launch, one 256-thread workgroup per
// problem (include/sgp_vfe_batch.h; the evaluation itself is vb_eval of sgp_vfe_batch.hpp).  Built into a library of its own,
// libsgp_vfe_batch_hip.so, beside libsgp_hip.so: the core library's surface stays what it was.  The one thing taken from the core at
// link time is sgp_ctx_device, for the context twin.  Nothing of sgp_dense.hip is used: a problem's matrices live in its workgroup's LDS.
#include "../../include/sgp_vfe_batch.h"
#include "sgp_vfe_batch.hpp"

namespace sgp {

// The small and the middle class are held to 256 registers, so that a CU takes two of their workgroups (their LDS allows it); the large
// class fills the LDS of a CU alone and may use the whole register file.
#if defined(SGP_AB_VFE_NO_REGISTER_BOUND)  // A/B knob (SGP_EXTRA_HIPCC_FLAGS, tools/vfe_batch_rates.py --tag): every class unbounded
#define SGP_VB_MIN_WAVES(MP) 1
#else
#define SGP_VB_MIN_WAVES(MP) ((MP) == 64 ? 1 : 2)
#endif
template <int KID, int MP>
__global__ __launch_bounds__(256, SGP_VB_MIN_WAVES(MP)) void vfe_batch_kernel(VbArgs a) {
  __shared__ VbShared<MP> sh;
  vb_eval<KID, MP>(sh, a, (int64_t)blockIdx.x);
}

}  // namespace sgp

using namespace sgp;

extern "C" size_t sgp_vfe_batch_workspace_bytes(int64_t P, int64_t N, int M, int d, int want_grad, int want_gz) {
  (void)want_grad, (void)want_gz;
  return vb_workspace_bytes(P, N, M, d);
}

// Workgroups of M's size class that one CU holds at a time, as the runtime counts them (registers and LDS of the loaded code object).
extern "C" int sgp_vfe_batch_occupancy(int M, int kernel_id) {
  const int chk = vb_check(1, 1, M, 1, kernel_id);
  if (chk != SGP_OK) return chk;
  return with_kid_class<16, 32, 64>(kernel_id, vb_size_class(M),
                                    [](auto kid, auto mp) { return wg_occupancy(vfe_batch_kernel<kid(), mp()>); });
}

extern "C" int sgp_vfe_eval_batch(const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const int* ix,
                                  const int* iy, const double* Z, int64_t z_stride, int64_t ldz, const int* iz, const double* theta,
                                  int64_t P, int64_t N, int M, int d, int kernel_id, double jitter, int want_grad, double* out, double* g_Z,
                                  int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  const int chk = vb_check(P, N, M, d, kernel_id);
  if (chk != SGP_OK && chk != SGP_ERR_DIM) return chk;
  if (!X || !Y || !Z || !theta || !out || !info || ldx < d || ldz < d || x_stride < 0 || y_stride < 0 || z_stride < 0 || !(jitter >= 0.0))
    return SGP_ERR_ARG;
  if (chk != SGP_OK) return chk;
  if (!ws || ws_bytes < vb_workspace_bytes(P, N, M, d)) return SGP_ERR_WORKSPACE;
  VbArgs a{};
  a.X = X, a.Y = Y, a.Z = Z, a.theta = theta;
  a.x_stride = x_stride, a.ldx = ldx, a.y_stride = y_stride, a.z_stride = z_stride, a.ldz = ldz;
  a.ix = ix, a.iy = iy, a.iz = iz;
  a.N = (int)N, a.M = M, a.d = d, a.want_grad = want_grad ? 1 : 0;
  a.jitter = jitter;
  a.out = out, a.gz = g_Z, a.info = info;
  with_kid_class<16, 32, 64>(kernel_id, vb_size_class(M), [&](auto kid, auto mp) {
    vfe_batch_kernel<kid(), mp()><<<dim3((unsigned)P), 256, 0, (hipStream_t)stream>>>(a);
  });
  return check_launch();
}

extern "C" int sgp_ctx_vfe_eval_batch(sgp_ctx* ctx, const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride,
                                      const int* ix, const int* iy, const double* Z, int64_t z_stride, int64_t ldz, const int* iz,
                                      const double* theta, int64_t P, int64_t N, int M, int d, int kernel_id, double jitter, int want_grad,
                                      double* out, double* g_Z, int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!ctx_device_matches(ctx)) return SGP_ERR_ARG;
  return sgp_vfe_eval_batch(X, x_stride, ldx, Y, y_stride, ix, iy, Z, z_stride, ldz, iz, theta, P, N, M, d, kernel_id, jitter, want_grad,
                            out, g_Z, info, ws, ws_bytes, stream);
}
