// C independent NUTS chains over the exact GP marginal likelihood, entirely on the device: ONE 256-thread workgroup per chain, the
// chain's whole problem in that workgroup's LDS (sgp_exact_batch.hpp), over any mix of data sets.  Thread 0 advances the chain's
// NutsState (sgp_nuts.hpp: nuts_step, resumable at every evaluation); all 256 threads evaluate at the position it asks for; thread 0
// applies ExactHmcTarget's density (sgp_exact_target.hpp).  Chains share nothing: no cooperative launch, no request words, no spins,
// no polling.  The one atomic is the "chains finished" counter, incremented once per chain when it finishes.
//
// A launch advances every unfinished chain by at most `evals_per_launch` evaluations and returns; the per-chain state (EnChain: the
// sampler's state, the last (logp, gradient) -- the position it belongs to is st.trial.q / st.cur.q -- and the device-clock stamp of the
// draw in flight) lives in the workspace in global memory, so the next launch resumes where this one stopped, in the middle of a tree
// if need be.  A launch ends after an evaluation's result is stored and before nuts_step consumes it: what is saved never depends on
// where the run was cut, and neither does any output but the per-draw seconds.
//
// Built into a library of its own, libsgp_exact_nuts_hip.so (include/sgp_exact_nuts.h), beside libsgp_hip.so: the core library's
// surface stays what it was.  The one thing taken from the core at link time is sgp_ctx_device, for the context twins.
//
// LDS per size class (static_assert below): the evaluation's image, the chain's own copy of y (the evaluation overwrites sh.yv with
// u = L^-1 y), a few result words -- and, for NP <= 64, the sampler's state for the length of a launch (copied in and out by all 256
// threads); at NP = 128 the image leaves no room for it and thread 0 works on the global copy.
#include "../../include/sgp_exact_nuts.h"
#include "sgp_exact_batch.hpp"
#include "sgp_exact_target.hpp"
#include "sgp_nuts.hpp"

namespace sgp {

constexpr int EN_ND = EB_MAXD + 2;
constexpr int EN_MAX_TREEDEPTH = NUTS_MAXDEPTH - 1;
constexpr int64_t EN_MAXC = EB_MAXP;  // one workgroup per chain; C x 19 kB of workspace and C x n_draws x (d + 2) sample indices stay far inside 64 bits
constexpr int EN_BAD_START = 1;       // info: the start position has no finite density
constexpr size_t EN_WS_HEAD = WG_WS_UNIT;  // the finished-chains counter, alone in its aligned unit
constexpr int EN_LDS_PER_CU = 163840;
enum { EN_EVAL = 1, EN_SKIP, EN_STOP, EN_DONE, EN_BAD };

struct EnChain {
  NutsState st;
  double lp, grad[EN_ND];     // the last evaluation's result, which the next nuts_step consumes
  unsigned long long t_draw;  // s_memrealtime (100 MHz) when the draw in flight began
  int finished, pad;
};
static_assert(sizeof(EnChain) % 8 == 0, "chains are copied as 8-byte words");

template <bool IN_LDS>
struct EnStateLds {
  NutsState st;
};
template <>
struct EnStateLds<false> {
  int unused;
};

struct EnWords {
  double q[EN_ND], v[EN_ND], th[EN_ND];  // the position asked for, exp(q), the evaluation's row
  double out[4], g[EN_ND];               // the evaluation's results
  double lp, grad[EN_ND];                // ... as the density the sampler sees
  unsigned long long t_draw;
  int info, cmd;
};
template <int NP>
struct EnShared {
  EnStateLds<(NP <= 64)> cache;
  double y[NP];  // the target, kept: sh.yv is overwritten by every evaluation
  EnWords w;
};
// two workgroups per CU in the two small classes (as exact_batch_kernel), one at NP = 128
static_assert(2 * (sizeof(EbShared<32>) + sizeof(EnShared<32>)) <= EN_LDS_PER_CU, "LDS: NP = 32");
static_assert(2 * (sizeof(EbShared<64>) + sizeof(EnShared<64>)) <= EN_LDS_PER_CU, "LDS: NP = 64");
static_assert(sizeof(EbShared<128>) + sizeof(EnShared<128>) <= EN_LDS_PER_CU, "LDS: NP = 128");
static_assert(sizeof(EbShared<128>) + sizeof(EnShared<128>) + sizeof(NutsState) > EN_LDS_PER_CU, "NP = 128: the state does not fit beside the image");

struct EnArgs {
  const double* X;
  int64_t x_stride, ldx;
  const double* Y;
  int64_t y_stride;
  const int *ix, *iy;
  int N, d;
  double jitter;
  double *samples, *stats, *seconds;  // [C, n_draws, d + 2], [C, n_draws, NST_COLS], [C, n_draws]
  long long *evaluations, *draws;     // [C]
  int* info;                          // [C]
  EnChain* chains;
  unsigned long long* finished;
  int evals_per_launch;
};

// Thread 0 between two evaluations: nuts_step consumes the last result and names the next position; the draw's device time; the range
// test and exp() of the position.
__device__ __forceinline__ int en_advance(NutsState* stp, EnWords* w, double* samples, double* stats, double* seconds, int d, double jitter) {
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
  if (r != NUTS_EVAL) return isfinite(st.cur.logp) ? EN_DONE : EN_BAD;
  if (!ext_in_range(qn, nd)) {  // zero density without an evaluation
    w->lp = -INFINITY;
    for (int i = 0; i < nd; ++i) w->grad[i] = 0.0;
    return EN_SKIP;
  }
  for (int i = 0; i < nd; ++i) w->q[i] = qn[i];
  ext_constrain(w->q, d, jitter, w->v, w->th);
  return EN_EVAL;
}

__global__ __launch_bounds__(64) void exact_nuts_begin_kernel(const double* __restrict__ q0, const unsigned long long* __restrict__ seed,
                                                              int64_t C, int d, int n_tune, int n_draws, int max_treedepth,
                                                              double step_scale, double target_accept, EnArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c == 0) *a.finished = 0ull;
  if (c >= C) return;
  EnChain& ch = a.chains[c];
  nuts_init(ch.st, d + 2, n_tune, n_draws, max_treedepth, step_scale, target_accept, seed[c], q0 + c * (d + 2));
  ch.lp = 0.0;
  for (int i = 0; i < EN_ND; ++i) ch.grad[i] = 0.0;
  ch.t_draw = 0ull;
  ch.finished = 0;
  ch.pad = 0;
  a.evaluations[c] = 0;
  a.draws[c] = 0;
  a.info[c] = 0;
}

// The evaluation as an out-of-line call, as sgp_small.hip's sampler has it (sm_eval_call).  Inlined into the chain loop beside
// nuts_step -- whose phase-space copies of 80 doubles want every register there is -- the kernel took 256 VGPRs + 120 AGPRs (one
// workgroup per CU in every class), and held to two workgroups per CU it spilled 132 VGPRs to scratch.  Out of line the evaluation
// keeps an allocation of its own: its scratch traffic is the callee-saved registers in its prologue and epilogue, none inside its
// loops (DESIGN 6e-3 has the resource lines of the builds).  The LDS objects live at namespace scope so that the callee addresses
// them directly (ds_* instructions) instead of through a generic pointer; each belongs to exactly one kernel instance.
template <int KID, int NP>
__shared__ EbShared<NP> g_en_sh;
template <int KID, int NP>
__shared__ EnShared<NP> g_en;

template <int KID, int NP>
__device__ __attribute__((noinline)) void en_eval_call(int N, int d) {
  EnWords& w = g_en<KID, NP>.w;
  eb_eval<KID, NP>(g_en_sh<KID, NP>, w.th, N, d, 1, w.out, w.g, &w.info);
}

// Registers: the two small classes are held to two workgroups per CU (exact_batch_kernel's occupancy; what does not fit is thread 0's
// sampler code, which spills a few values to scratch); NP = 128 has the CU to itself anyway.
template <int KID, int NP>
__global__ __launch_bounds__(256, (NP <= 64 ? 2 : 1)) void exact_nuts_kernel(EnArgs a) {
  constexpr bool ST_LDS = NP <= 64;
  EbShared<NP>& sh = g_en_sh<KID, NP>;
  EnShared<NP>& en = g_en<KID, NP>;
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x, N = a.N, d = a.d, nd = d + 2;
  EnChain* ch = a.chains + c;
  if (ch->finished) return;  // (written by an earlier launch: the same answer in every thread)
  NutsState* stp;
  if constexpr (ST_LDS) {
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&ch->st);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(&en.cache.st);
    for (int e = tid; e < (int)(sizeof(NutsState) / 8); e += 256) dst[e] = src[e];
    stp = &en.cache.st;
  } else {
    stp = &ch->st;
  }
  NutsState& st = *stp;
  eb_load<NP>(sh, en.y, a.X + (int64_t)(a.ix ? a.ix[c] : 0) * a.x_stride, a.ldx, a.Y + (int64_t)(a.iy ? a.iy[c] : 0) * a.y_stride, N, d);
  if (tid == 0) {
    en.w.lp = ch->lp;
    for (int i = 0; i < EN_ND; ++i) en.w.grad[i] = ch->grad[i];
  }
  __syncthreads();
  const int n_draws = st.n_draws, Nr = round_up(N, 16);
  double* samples = a.samples + c * n_draws * nd;
  double* stats = a.stats + c * n_draws * NST_COLS;
  double* seconds = a.seconds + c * n_draws;
  if (tid == 0) en.w.t_draw = st.phase == NS_INIT ? __builtin_amdgcn_s_memrealtime() : ch->t_draw;

  int cm;
  for (int ev = 0;; ++ev) {
    if (tid == 0) en.w.cmd = ev < a.evals_per_launch ? en_advance(stp, &en.w, samples, stats, seconds, d, a.jitter) : EN_STOP;
    __syncthreads();
    cm = en.w.cmd;
    if (cm != EN_EVAL) {
      if (cm != EN_SKIP) break;
      __syncthreads();  // every thread has read cmd before thread 0 writes the next one
      continue;
    }
    for (int i = tid; i < Nr; i += 256) sh.yv[i] = en.y[i];
    en_eval_call<KID, NP>(N, d);
    __syncthreads();
    if (tid == 0) en.w.lp = ext_logp_grad(en.w.q, en.w.v, d, en.w.out[0], en.w.g, en.w.info, en.w.grad);
  }

  // ---- the launch ends: save the chain (cm is EN_STOP, EN_DONE or EN_BAD, the same in every thread) ----
  if (tid == 0) {
    ch->lp = en.w.lp;
    for (int i = 0; i < EN_ND; ++i) ch->grad[i] = en.w.grad[i];
    ch->t_draw = en.w.t_draw;
    if (cm != EN_STOP) {
      a.evaluations[c] = (long long)st.n_leapfrog;
      a.draws[c] = st.it;
      a.info[c] = cm == EN_BAD ? EN_BAD_START : 0;
      ch->finished = 1;
      atomicAdd(a.finished, 1ull);
    }
  }
  if (cm == EN_BAD) {  // nothing was sampled: the chain's rows are NaN
    const double nan = __builtin_nan("");
    for (int64_t e = tid; e < (int64_t)n_draws * nd; e += 256) samples[e] = nan;
    for (int64_t e = tid; e < (int64_t)n_draws * NST_COLS; e += 256) stats[e] = nan;
    for (int64_t e = tid; e < n_draws; e += 256) seconds[e] = nan;
  }
  if constexpr (ST_LDS) {
    __syncthreads();
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&en.cache.st);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(&ch->st);
    for (int e = tid; e < (int)(sizeof(NutsState) / 8); e += 256) dst[e] = src[e];
  }
}

}  // namespace sgp

using namespace sgp;

static int exact_nuts_check(int64_t C, int N, int d, int kernel_id) {
  if (C <= 0 || N <= 0 || d <= 0) return SGP_ERR_ARG;
  if (kernel_id < 0 || kernel_id > SGP_KERNEL_MATERN52) return SGP_ERR_ARG;  // composite kernels: out of scope, as in sgp_exact_eval_batch
  if (N > EB_MAXN || d > EB_MAXD || C > EN_MAXC) return SGP_ERR_DIM;
  return SGP_OK;
}

extern "C" size_t sgp_exact_nuts_batch_workspace_bytes(int64_t C, int N, int d) {
  return exact_nuts_check(C, N, d, 0) == SGP_OK ? EN_WS_HEAD + (size_t)C * sizeof(EnChain) : 0;
}

// Workgroups (= chains) of N's size class that one CU holds at a time, as the runtime counts them.
extern "C" int sgp_exact_nuts_batch_occupancy(int N, int kernel_id) {
  const int chk = exact_nuts_check(1, N, 1, kernel_id);
  if (chk != SGP_OK) return chk;
  return with_kid_class<32, 64, 128>(kernel_id, eb_size_class(N),
                                     [](auto kid, auto np) { return wg_occupancy(exact_nuts_kernel<kid(), np()>); });
}

static EnArgs en_args(double* samples, double* stats, double* seconds, int64_t* evaluations, int64_t* draws, int* info, void* ws) {
  EnArgs a{};
  a.samples = samples;
  a.stats = stats;
  a.seconds = seconds;
  a.evaluations = reinterpret_cast<long long*>(evaluations);
  a.draws = reinterpret_cast<long long*>(draws);
  a.info = info;
  a.finished = reinterpret_cast<unsigned long long*>(ws);
  a.chains = reinterpret_cast<EnChain*>(static_cast<char*>(ws) + EN_WS_HEAD);
  return a;
}

extern "C" int sgp_exact_nuts_batch_begin(const double* q0, const uint64_t* seed, int64_t C, int N, int d, int kernel_id, int n_tune,
                                          int n_draws, int max_treedepth, double step_scale, double target_accept, double* samples,
                                          double* stats, double* seconds, int64_t* evaluations, int64_t* draws, int* info, void* ws,
                                          size_t ws_bytes, sgp_stream_t stream) {
  const int chk = exact_nuts_check(C, N, d, kernel_id);
  if (chk != SGP_OK && chk != SGP_ERR_DIM) return chk;
  if (!q0 || !seed || !samples || !stats || !seconds || !evaluations || !draws || !info ||
      !nuts_params_ok(n_tune, n_draws, max_treedepth, EN_MAX_TREEDEPTH, step_scale, target_accept))
    return SGP_ERR_ARG;
  if (chk != SGP_OK) return chk;
  if (!ws || ws_bytes < sgp_exact_nuts_batch_workspace_bytes(C, N, d)) return SGP_ERR_WORKSPACE;
  const EnArgs a = en_args(samples, stats, seconds, evaluations, draws, info, ws);
  exact_nuts_begin_kernel<<<dim3((unsigned)((C + 63) / 64)), 64, 0, (hipStream_t)stream>>>(
      q0, reinterpret_cast<const unsigned long long*>(seed), C, d, n_tune, n_draws, max_treedepth, step_scale, target_accept, a);
  return check_launch();
}

extern "C" int sgp_exact_nuts_batch_advance(const double* X, int64_t x_stride, int64_t ldx, const double* Y, int64_t y_stride, const int* ix,
                                            const int* iy, int64_t C, int N, int d, int kernel_id, double jitter, double* samples,
                                            double* stats, double* seconds, int64_t* evaluations, int64_t* draws, int* info,
                                            int evals_per_launch, int64_t* finished, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  const int chk = exact_nuts_check(C, N, d, kernel_id);
  if (chk != SGP_OK && chk != SGP_ERR_DIM) return chk;
  if (!X || !Y || !samples || !stats || !seconds || !evaluations || !draws || !info || !finished || ldx < d || x_stride < 0 ||
      y_stride < 0 || evals_per_launch <= 0 || !(jitter >= 0.0))
    return SGP_ERR_ARG;
  if (chk != SGP_OK) return chk;
  if (!ws || ws_bytes < sgp_exact_nuts_batch_workspace_bytes(C, N, d)) return SGP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  EnArgs a = en_args(samples, stats, seconds, evaluations, draws, info, ws);
  a.X = X, a.x_stride = x_stride, a.ldx = ldx, a.Y = Y, a.y_stride = y_stride, a.ix = ix, a.iy = iy;
  a.N = N, a.d = d, a.jitter = jitter, a.evals_per_launch = evals_per_launch;
  with_kid_class<32, 64, 128>(kernel_id, eb_size_class(N), [&](auto kid, auto np) {
    exact_nuts_kernel<kid(), np()><<<dim3((unsigned)C), 256, 0, st>>>(a);
  });
  return nuts_read_finished(a.finished, finished, st);
}

extern "C" int sgp_ctx_exact_nuts_batch_begin(sgp_ctx* ctx, const double* q0, const uint64_t* seed, int64_t C, int N, int d, int kernel_id,
                                              int n_tune, int n_draws, int max_treedepth, double step_scale, double target_accept,
                                              double* samples, double* stats, double* seconds, int64_t* evaluations, int64_t* draws,
                                              int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!ctx_device_matches(ctx)) return SGP_ERR_ARG;
  return sgp_exact_nuts_batch_begin(q0, seed, C, N, d, kernel_id, n_tune, n_draws, max_treedepth, step_scale, target_accept, samples, stats,
                                    seconds, evaluations, draws, info, ws, ws_bytes, stream);
}
extern "C" int sgp_ctx_exact_nuts_batch_advance(sgp_ctx* ctx, const double* X, int64_t x_stride, int64_t ldx, const double* Y,
                                                int64_t y_stride, const int* ix, const int* iy, int64_t C, int N, int d, int kernel_id,
                                                double jitter, double* samples, double* stats, double* seconds, int64_t* evaluations,
                                                int64_t* draws, int* info, int evals_per_launch, int64_t* finished, void* ws,
                                                size_t ws_bytes, sgp_stream_t stream) {
  if (!ctx_device_matches(ctx)) return SGP_ERR_ARG;
  return sgp_exact_nuts_batch_advance(X, x_stride, ldx, Y, y_stride, ix, iy, C, N, d, kernel_id, jitter, samples, stats, seconds,
                                      evaluations, draws, info, evals_per_launch, finished, ws, ws_bytes, stream);
}
