// C independent NUTS chains over the collapsed (Titsias / VFE) sparse-GP bound at fixed inducing inputs, entirely on the device: ONE
// 256-thread workgroup per chain, over any mix of data sets and inducing sets.  Thread 0 advances the chain's NutsState (sgp_nuts.hpp:
// nuts_step, resumable at every evaluation); all 256 threads run vb_eval (sgp_vfe_batch.hpp) at the position it asks for; thread 0
// applies HmcTarget's density (sgp_exact_target.hpp: the priors, the log-Jacobians and the chain rule are those of the exact sampler,
// the jitter goes to K_uu and not to the noise).  Chains share nothing: no cooperative launch, no request words, no spins, no polling.
// The one atomic is the "chains finished" counter, incremented once per chain when it finishes.
//
// vb_eval is used as sgp_vfe_eval_batch has it, unchanged: it reads its theta row from VbArgs::theta and writes `out` and `info` through
// VbArgs, so every chain owns a theta row, an `out` row and an `info` word in the workspace, and the VbArgs of a launch points at those
// arrays with p = the chain's index.  Thread 0 writes the row before the barrier that precedes the evaluation and reads the results
// after the barrier that follows it: a few hundred nanoseconds of round trips against an evaluation of 60 us and more.
//
// A launch advances every unfinished chain by at most `evals_per_launch` evaluations and returns; the per-chain state (VnChain) lives in
// the workspace, so the next launch resumes where this one stopped, in the middle of a tree if need be.  A launch ends after an
// evaluation's result is stored and before nuts_step consumes it: what is saved never depends on where the run was cut, and neither
// does any output but the per-draw seconds.
//
// vn_advance and the chain save / restore repeat sgp_exact_nuts.hip's en_advance and its kernel frame (about 25 lines each): a helper
// shared into that translation unit changes its register allocation, so a fix to either copy has to be made in the other.
//
// Built into a library of its own, libsgp_vfe_nuts_hip.so (include/sgp_vfe_nuts.h), beside libsgp_hip.so.  The one thing taken from the
// core at link time is sgp_ctx_device, for the context twins.
//
// LDS per size class (static_assert below): vb_eval's image, the sampler's words and, in every class, the sampler's state for the length
// of a launch (copied in and out by all 256 threads) -- two workgroups per CU in the classes 16 and 32 as for sgp_vfe_eval_batch; at
// class 64 the state (18 992 bytes) takes what the image (143 976 bytes) leaves of the CU's 163 840, with 600 bytes to spare.
#include "../../include/sgp_vfe_nuts.h"
#include "sgp_vfe_batch.hpp"
#include "sgp_exact_target.hpp"
#include "sgp_nuts.hpp"

namespace sgp {

constexpr int VN_ND = VB_MAXD + 2;
constexpr int VN_MAX_TREEDEPTH = NUTS_MAXDEPTH - 1;
constexpr int VN_BAD_START = SGP_VFE_NUTS_BAD_START;  // info: the start position has no finite density
constexpr size_t VN_WS_HEAD = WG_WS_UNIT;            // the finished-chains counter, alone in its aligned unit
constexpr int VN_LDS_PER_CU = 163840;
enum { VN_EVAL = 1, VN_SKIP, VN_STOP, VN_DONE, VN_BAD };
static_assert(VB_MAXD == EXT_MAXD, "the density transform and the evaluation agree on the number of lengthscales");

struct VnChain {
  NutsState st;
  double lp, grad[VN_ND];     // the last evaluation's result, which the next nuts_step consumes
  unsigned long long t_draw;  // s_memrealtime (100 MHz) when the draw in flight began
  int finished, pad;
};
static_assert(sizeof(VnChain) % 8 == 0 && sizeof(NutsState) % 8 == 0, "chains are copied as 8-byte words");

struct VnWords {
  double q[VN_ND], v[VN_ND];  // the position asked for and exp(q); the evaluation's row goes to the chain's theta row in the workspace
  double lp, grad[VN_ND];     // the density the sampler sees
  unsigned long long t_draw;
  int cmd, pad;
};
struct VnShared {
  NutsState st;  // the chain's state, cached for the length of a launch
  VnWords w;
};
// two workgroups per CU in the two small classes (as vfe_batch_kernel), one at class 64
static_assert(2 * (sizeof(VbShared<16>) + sizeof(VnShared)) <= VN_LDS_PER_CU, "LDS: class 16");
static_assert(2 * (sizeof(VbShared<32>) + sizeof(VnShared)) <= VN_LDS_PER_CU, "LDS: class 32");
static_assert(sizeof(VbShared<64>) + sizeof(VnShared) <= VN_LDS_PER_CU, "LDS: class 64");

// The workspace: [counter unit | C chains | C theta rows of d + 2 | C out rows of d + 5 | C info words], each part 8-byte aligned
struct VnLayout {
  size_t chains, theta, out, info, total;
};
inline VnLayout vn_layout(int64_t C, int d) {
  VnLayout l;
  l.chains = VN_WS_HEAD;
  l.theta = l.chains + (size_t)C * sizeof(VnChain);
  l.out = l.theta + (size_t)C * (size_t)(d + 2) * sizeof(double);
  l.info = l.out + (size_t)C * (size_t)(d + 5) * sizeof(double);
  l.total = (l.info + (size_t)C * sizeof(int) + WG_WS_UNIT - 1) / WG_WS_UNIT * WG_WS_UNIT;
  return l;
}

struct VnArgs {
  VbArgs vb;                          // the evaluation's view: theta / out / info are the per-chain arrays of the workspace, gz is null
  double *samples, *stats, *seconds;  // [C, n_draws, d + 2], [C, n_draws, NST_COLS], [C, n_draws]
  long long *evaluations, *draws;     // [C]
  int* info;                          // [C]
  VnChain* chains;
  double *theta, *out;                // vb.theta and vb.out again, writable / for thread 0
  int* einfo;                         // vb.info
  unsigned long long* finished;
  int evals_per_launch;
};

// Thread 0 between two evaluations: nuts_step consumes the last result and names the next position; the draw's device time; the range
// test and exp() of the position; the evaluation's row [ls | sig_f^2 | sig_n^2] into the chain's theta row.  (en_advance of
// sgp_exact_nuts.hip, with the row in global memory.)
__device__ __forceinline__ int vn_advance(NutsState* stp, VnWords* w, double* th, double* samples, double* stats, double* seconds, int d) {
  NutsState& st = *stp;
  const int nd = d + 2;
  const double* qn = nullptr;
  const int it0 = st.it;
  const int r = nuts_step(st, w->lp, w->grad, &qn, samples, stats);
  if (st.it != it0) {  // a draw has finished: its device time
    const unsigned long long now = __builtin_amdgcn_s_memrealtime();
    if (it0 >= st.n_tune) seconds[it0 - st.n_tune] = (double)(now - w->t_draw) * 1e-8;
    w->t_draw = now;
  }
  if (r != NUTS_EVAL) return isfinite(st.cur.logp) ? VN_DONE : VN_BAD;
  if (!ext_in_range(qn, nd)) {  // zero density without an evaluation
    w->lp = -INFINITY;
    for (int i = 0; i < nd; ++i) w->grad[i] = 0.0;
    return VN_SKIP;
  }
  for (int i = 0; i < nd; ++i) w->q[i] = qn[i];
  ext_constrain(w->q, d, 0.0, w->v, th);
  return VN_EVAL;
}

__global__ __launch_bounds__(64) void vfe_nuts_begin_kernel(const double* __restrict__ q0, const unsigned long long* __restrict__ seed,
                                                            int64_t C, int d, int n_tune, int n_draws, int max_treedepth,
                                                            double step_scale, double target_accept, VnArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c == 0) *a.finished = 0ull;
  if (c >= C) return;
  VnChain& ch = a.chains[c];
  nuts_init(ch.st, d + 2, n_tune, n_draws, max_treedepth, step_scale, target_accept, seed[c], q0 + c * (d + 2));
  ch.lp = 0.0;
  for (int i = 0; i < VN_ND; ++i) ch.grad[i] = 0.0;
  ch.t_draw = 0ull;
  ch.finished = 0;
  ch.pad = 0;
  for (int i = 0; i < d + 2; ++i) a.theta[c * (d + 2) + i] = 1.0;
  for (int i = 0; i < d + 5; ++i) a.out[c * (d + 5) + i] = 0.0;
  a.einfo[c] = 0;
  a.evaluations[c] = 0;
  a.draws[c] = 0;
  a.info[c] = 0;
}

// The evaluation as an out-of-line call and the LDS objects at namespace scope, as sgp_exact_nuts.hip has them (en_eval_call) and for
// the reason written there: inlined beside nuts_step the evaluation shares its register allocation with the sampler's phase-space
// copies; out of line it keeps an allocation of its own and addresses its image directly (ds_* instructions).
template <int KID, int MP>
__shared__ VbShared<MP> g_vn_sh;
template <int KID, int MP>
__shared__ VnShared g_vn;

template <int KID, int MP>
__device__ __attribute__((noinline)) void vn_eval_call(const VbArgs* a, int64_t c) {
  vb_eval<KID, MP>(g_vn_sh<KID, MP>, *a, c);
}

// Registers: the two small classes are held to two workgroups per CU (vfe_batch_kernel's occupancy); class 64 has the CU to itself.
template <int KID, int MP>
__global__ __launch_bounds__(256, (MP <= 32 ? 2 : 1)) void vfe_nuts_kernel(VnArgs a) {
  VnShared& vn = g_vn<KID, MP>;
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x, d = a.vb.d, nd = d + 2;
  VnChain* ch = a.chains + c;
  if (ch->finished) return;  // (written by an earlier launch: the same answer in every thread)
  {
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&ch->st);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(&vn.st);
    for (int e = tid; e < (int)(sizeof(NutsState) / 8); e += 256) dst[e] = src[e];
  }
  NutsState* stp = &vn.st;
  NutsState& st = *stp;
  if (tid == 0) {
    vn.w.lp = ch->lp;
    for (int i = 0; i < VN_ND; ++i) vn.w.grad[i] = ch->grad[i];
  }
  __syncthreads();
  const int n_draws = st.n_draws;
  double* samples = a.samples + c * n_draws * nd;
  double* stats = a.stats + c * n_draws * NST_COLS;
  double* seconds = a.seconds + c * n_draws;
  double* th = a.theta + c * nd;
  const double* out = a.out + c * (d + 5);
  if (tid == 0) vn.w.t_draw = st.phase == NS_INIT ? __builtin_amdgcn_s_memrealtime() : ch->t_draw;

  int cm;
  for (int ev = 0;; ++ev) {
    if (tid == 0) vn.w.cmd = ev < a.evals_per_launch ? vn_advance(stp, &vn.w, th, samples, stats, seconds, d) : VN_STOP;
    __syncthreads();  // cmd, and thread 0's theta row, are visible to the workgroup
    cm = vn.w.cmd;
    if (cm != VN_EVAL) {
      if (cm != VN_SKIP) break;
      __syncthreads();  // every thread has read cmd before thread 0 writes the next one
      continue;
    }
    vn_eval_call<KID, MP>(&a.vb, c);
    __syncthreads();  // out / info of this chain are written; every thread is through with the image
    if (tid == 0) vn.w.lp = ext_logp_grad(vn.w.q, vn.w.v, d, out[0], out + 1, a.einfo[c], vn.w.grad);
  }

  // ---- the launch ends: save the chain (cm is VN_STOP, VN_DONE or VN_BAD, the same in every thread) ----
  if (tid == 0) {
    ch->lp = vn.w.lp;
    for (int i = 0; i < VN_ND; ++i) ch->grad[i] = vn.w.grad[i];
    ch->t_draw = vn.w.t_draw;
    if (cm != VN_STOP) {
      a.evaluations[c] = (long long)st.n_leapfrog;
      a.draws[c] = st.it;
      a.info[c] = cm == VN_BAD ? VN_BAD_START : 0;
      ch->finished = 1;
      atomicAdd(a.finished, 1ull);
    }
  }
  if (cm == VN_BAD) {  // nothing was sampled: the chain's rows are NaN
    const double nan = __builtin_nan("");
    for (int64_t e = tid; e < (int64_t)n_draws * nd; e += 256) samples[e] = nan;
    for (int64_t e = tid; e < (int64_t)n_draws * NST_COLS; e += 256) stats[e] = nan;
    for (int64_t e = tid; e < n_draws; e += 256) seconds[e] = nan;
  }
  __syncthreads();
  {
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&vn.st);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(&ch->st);
    for (int e = tid; e < (int)(sizeof(NutsState) / 8); e += 256) dst[e] = src[e];
  }
}

}  // namespace sgp

using namespace sgp;

extern "C" size_t sgp_vfe_nuts_batch_workspace_bytes(int64_t C, int64_t N, int M, int d) {
  return vb_check(C, N, M, d, 0) == SGP_OK ? vn_layout(C, d).total : 0;
}

// Workgroups (= chains) of M's size class that one CU holds at a time, as the runtime counts them.
extern "C" int sgp_vfe_nuts_batch_occupancy(int M, int kernel_id) {
  const int chk = vb_check(1, 1, M, 1, kernel_id);
  if (chk != SGP_OK) return chk;
  return with_kid_class<16, 32, 64>(kernel_id, vb_size_class(M),
                                    [](auto kid, auto mp) { return wg_occupancy(vfe_nuts_kernel<kid(), mp()>); });
}

static VnArgs vn_args(int64_t C, int d, double* samples, double* stats, double* seconds, int64_t* evaluations, int64_t* draws, int* info,
                      void* ws) {
  const VnLayout l = vn_layout(C, d);
  char* base = static_cast<char*>(ws);
  VnArgs a{};
  a.samples = samples;
  a.stats = stats;
  a.seconds = seconds;
  a.evaluations = reinterpret_cast<long long*>(evaluations);
  a.draws = reinterpret_cast<long long*>(draws);
  a.info = info;
  a.finished = reinterpret_cast<unsigned long long*>(base);
  a.chains = reinterpret_cast<VnChain*>(base + l.chains);
  a.theta = reinterpret_cast<double*>(base + l.theta);
  a.out = reinterpret_cast<double*>(base + l.out);
  a.einfo = reinterpret_cast<int*>(base + l.info);
  return a;
}

extern "C" int sgp_vfe_nuts_batch_begin(const double* q0, const uint64_t* seed, int64_t C, int64_t N, int M, int d, int kernel_id,
                                        int n_tune, int n_draws, int max_treedepth, double step_scale, double target_accept,
                                        double* samples, double* stats, double* seconds, int64_t* evaluations, int64_t* draws, int* info,
                                        void* ws, size_t ws_bytes, sgp_stream_t stream) {
  const int chk = vb_check(C, N, M, d, kernel_id);
  if (chk != SGP_OK && chk != SGP_ERR_DIM) return chk;
  if (!q0 || !seed || !samples || !stats || !seconds || !evaluations || !draws || !info ||
      !nuts_params_ok(n_tune, n_draws, max_treedepth, VN_MAX_TREEDEPTH, step_scale, target_accept))
    return SGP_ERR_ARG;
  if (chk != SGP_OK) return chk;
  if (!ws || ws_bytes < sgp_vfe_nuts_batch_workspace_bytes(C, N, M, d)) return SGP_ERR_WORKSPACE;
  const VnArgs a = vn_args(C, d, samples, stats, seconds, evaluations, draws, info, ws);
  vfe_nuts_begin_kernel<<<dim3((unsigned)((C + 63) / 64)), 64, 0, (hipStream_t)stream>>>(
      q0, reinterpret_cast<const unsigned long long*>(seed), C, d, n_tune, n_draws, max_treedepth, step_scale, target_accept, a);
  return check_launch();
}

extern "C" int sgp_vfe_nuts_batch_advance(const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const int* ix,
                                          const int* iy, const double* Z, int64_t z_stride, int64_t ldz, const int* iz, int64_t C,
                                          int64_t N, int M, int d, int kernel_id, double jitter, double* samples, double* stats,
                                          double* seconds, int64_t* evaluations, int64_t* draws, int* info, int evals_per_launch,
                                          int64_t* finished, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  const int chk = vb_check(C, N, M, d, kernel_id);
  if (chk != SGP_OK && chk != SGP_ERR_DIM) return chk;
  if (!X || !Y || !Z || !samples || !stats || !seconds || !evaluations || !draws || !info || !finished || ldx < d || ldz < d ||
      x_stride < 0 || y_stride < 0 || z_stride < 0 || evals_per_launch <= 0 || !(jitter >= 0.0))
    return SGP_ERR_ARG;
  if (chk != SGP_OK) return chk;
  if (!ws || ws_bytes < sgp_vfe_nuts_batch_workspace_bytes(C, N, M, d)) return SGP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  VnArgs a = vn_args(C, d, samples, stats, seconds, evaluations, draws, info, ws);
  a.vb.X = X, a.vb.Y = Y, a.vb.Z = Z, a.vb.theta = a.theta;
  a.vb.x_stride = x_stride, a.vb.ldx = ldx, a.vb.y_stride = y_stride, a.vb.z_stride = z_stride, a.vb.ldz = ldz;
  a.vb.ix = ix, a.vb.iy = iy, a.vb.iz = iz;
  a.vb.N = (int)N, a.vb.M = M, a.vb.d = d, a.vb.want_grad = 1;
  a.vb.jitter = jitter;
  a.vb.out = a.out, a.vb.gz = nullptr, a.vb.info = a.einfo;
  a.evals_per_launch = evals_per_launch;
  with_kid_class<16, 32, 64>(kernel_id, vb_size_class(M), [&](auto kid, auto mp) {
    vfe_nuts_kernel<kid(), mp()><<<dim3((unsigned)C), 256, 0, st>>>(a);
  });
  return nuts_read_finished(a.finished, finished, st);
}

extern "C" int sgp_ctx_vfe_nuts_batch_begin(sgp_ctx* ctx, const double* q0, const uint64_t* seed, int64_t C, int64_t N, int M, int d,
                                            int kernel_id, int n_tune, int n_draws, int max_treedepth, double step_scale,
                                            double target_accept, double* samples, double* stats, double* seconds, int64_t* evaluations,
                                            int64_t* draws, int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!ctx_device_matches(ctx)) return SGP_ERR_ARG;
  return sgp_vfe_nuts_batch_begin(q0, seed, C, N, M, d, kernel_id, n_tune, n_draws, max_treedepth, step_scale, target_accept, samples,
                                  stats, seconds, evaluations, draws, info, ws, ws_bytes, stream);
}
extern "C" int sgp_ctx_vfe_nuts_batch_advance(sgp_ctx* ctx, const double* X, int64_t x_stride, int64_t ldx, const double* Y,
                                              int64_t y_stride, const int* ix, const int* iy, const double* Z, int64_t z_stride,
                                              int64_t ldz, const int* iz, int64_t C, int64_t N, int M, int d, int kernel_id, double jitter,
                                              double* samples, double* stats, double* seconds, int64_t* evaluations, int64_t* draws,
                                              int* info, int evals_per_launch, int64_t* finished, void* ws, size_t ws_bytes,
                                              sgp_stream_t stream) {
  if (!ctx_device_matches(ctx)) return SGP_ERR_ARG;
  return sgp_vfe_nuts_batch_advance(X, x_stride, ldx, Y, y_stride, ix, iy, Z, z_stride, ldz, iz, C, N, M, d, kernel_id, jitter, samples,
                                    stats, seconds, evaluations, draws, info, evals_per_launch, finished, ws, ws_bytes, stream);
}
