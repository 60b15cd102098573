// What the one-workgroup-per-problem kernels share: sgp_exact_batch.hpp (the batched exact marginal likelihood, the batched NUTS, the
// batched predictive) and sgp_vfe_batch.hpp (the batched collapsed bound) keep a whole dense problem in their workgroup's LDS.  Here
// are the layout their images are written for, the unit their workspace queries answer with, and the host-side frame of their entry
// points.  The panel Cholesky and the triangular inverse are NOT here: each header keeps its own (vb_chol / vb_invert are eb_factor's
// and eb_invert's line for line).  One shared copy compiles to other machine code in these kernels and is slower in all four
// libraries (profiles/wg_dense_refactor_rates.json), so a fix to either copy has to be made in the other as well.
//
// The layout.  An image is n x n (n a multiple of 16, identity in the padding) inside rows of n_class + 2 doubles, n_class the size
// class (a power of two from 16 to 128).  Row stride n_class + 2 = 2 (mod 32) eight-byte slots:
//   * "16 rows x 4 consecutive columns" (MFMA operands whose contraction index runs along a row: the rank-16 trailing update, the Inv
//     operand of the triangular inversion) -- a 32-lane group touches slots 2 r + c, r < 16, c < 2: all distinct;
//   * "4 rows x 16 consecutive columns" (contraction index running down a column: the A^-1 tiles of the exact gradient, the dominant
//     N^3 / 3 phase, and A A^T of the collapsed bound) -- the four lane groups l4 of an MFMA take the rows k0 + kperm + s,
//     kperm = 8 (l4 & 1) + 4 (l4 >> 1) = {0, 8, 4, 12}, instead of k0 + 4 s + {0, 1, 2, 3}, so the two rows of a 32-lane group are 8
//     apart = 16 slots: all distinct.  (Any fixed assignment of the 16 rows to the 16 (group, step) pairs is the same sum in another,
//     still fixed, order.)
//   * row reads are contiguous; the thread-per-row panel solves and the accumulator-tile loads and stores (two adjacent rows per lane
//     group) are 2-way -- 32 eight-byte accesses per thread and panel, off the MFMA phases.
// Every sum has a fixed order and depends on nothing outside the problem: the same bits on every call, stream and batch.
//
// The first part of this header is plain C++: a host program can include it without HIP (tests/native/vfe_batch_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace sgp {

// What a workspace query of these libraries answers for a supported shape when the kernel keeps everything in LDS: one aligned unit,
// so that "0 = unsupported shape" and "a non-NULL buffer of at least that size" hold as for every other entry point.
constexpr size_t WG_WS_UNIT = 256;

}  // namespace sgp

#if defined(__HIPCC__)
#include <type_traits>
#include "sgp_common.hpp"

namespace sgp {

// ---- the host-side frame of an entry point: kernel<KID, class> is picked, launched and asked for its occupancy in one place ----

// f(kid, cls) with the kernel id (RBF, Matern-3/2, Matern-5/2: the callers have refused every other) and the size class `cls`, one
// of C0 < C1 < C2, as std::integral_constant: inside f, kernel<kid(), cls()> names the instantiation.
template <int C0, int C1, int C2, class F>
inline auto with_kid_class(int kernel_id, int cls, F&& f) {
  auto by_class = [&](auto kid) {
    if (cls == C0) return f(kid, std::integral_constant<int, C0>{});
    if (cls == C1) return f(kid, std::integral_constant<int, C1>{});
    return f(kid, std::integral_constant<int, C2>{});
  };
  switch (kernel_id) {
    case SGP_KERNEL_RBF: return by_class(std::integral_constant<int, SGP_KERNEL_RBF>{});
    case SGP_KERNEL_MATERN32: return by_class(std::integral_constant<int, SGP_KERNEL_MATERN32>{});
    default: return by_class(std::integral_constant<int, SGP_KERNEL_MATERN52>{});
  }
}

// Workgroups of 256 threads of `kernel` that one CU holds at a time, as the runtime counts them (registers and LDS of the loaded code
// object), or SGP_ERR_LAUNCH
template <class K>
inline int wg_occupancy(K kernel) {
  int n = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, 0) == hipSuccess ? n : SGP_ERR_LAUNCH;
}

// The context twins of these libraries: their kernels read no context option, so what a context means is the device it belongs to.
// NULL (the default context) follows the caller; with no device at all the argument checks and the launch report that.
inline bool ctx_device_matches(const sgp_ctx* ctx) {
  int dev = -1;
  return !ctx || hipGetDevice(&dev) != hipSuccess || dev == sgp_ctx_device(ctx);
}

// ---- the host half the two device-resident samplers (sgp_exact_nuts.hip, sgp_vfe_nuts.hip) share ----

// The sampler parameters a *_nuts_batch_begin accepts (a NaN fails every comparison); `depth_limit` is the library's own
inline bool nuts_params_ok(int n_tune, int n_draws, int max_treedepth, int depth_limit, double step_scale, double target_accept) {
  return n_tune >= 0 && n_draws >= 0 && max_treedepth >= 0 && max_treedepth <= depth_limit && step_scale > 0.0 && target_accept > 0.0 &&
         target_accept < 1.0;
}

// The tail of a *_nuts_batch_advance: the launch's status, then the one read-back of a launch -- how many chains have finished
inline int nuts_read_finished(const unsigned long long* counter, int64_t* finished, hipStream_t st) {
  if (check_launch() != SGP_OK) return SGP_ERR_LAUNCH;
  unsigned long long done = 0;
  if (hipMemcpyAsync(&done, counter, sizeof(done), hipMemcpyDeviceToHost, st) != hipSuccess) return SGP_ERR_LAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return SGP_ERR_LAUNCH;
  *finished = (int64_t)done;
  return SGP_OK;
}

}  // namespace sgp
#endif  // __HIPCC__
