// The row pass of SGPMC with a non-conjugate likelihood (include/sgp.h: sgp_sgpmc_lik_rows): from T = K'_fu L^-T of the whitened rows
// layout, per datum the conditional moments  mu_n = a_n.v,  var_n = sf2 - |a_n|^2  (a_n = sf2 T_n), the likelihood layer of
// sgp_lik.hpp, and the two M-sized adjoints  g = sum_n dmu_n a_n,  G = sum_n dv_n a_n a_n^T.  A user of the host-side frame of
// sgp_stream.hpp: the plan is rows_plan, the start of the pass stream_rows_start (both shared with sgp_sgpmc_mc.hip); the contraction,
// tpart_kernel and the fixed-order reductions are sgp_suffstats_fwd.hip's own:
//   stream_rows_start                                         prologue, R = L^-T, assembly, T = K' R (the unweighted T^T T of the Gaussian path is not run)
//   sgpmc_lik_rows_kernel                                     reads T once: moments + likelihood, dmu, dv, [sum ell | sum ds2 | sum dv]
//                                                             (closed by last_block_sums of sgp_common.hpp; zero_ints ahead of it)
//   -- a value-only call ends here --
//   tpart_kernel(ys := dmu) + the b reduction                 g
//   sgpmc_lik_scale_kernel(+1), contraction, slab reduction   T_n <- sqrt(-dv_n) T_n;  G = -sf2^2 S^T S  (dv <= 0: log-concave likelihoods)
//   sgpmc_lik_scale_kernel(-1)                                T_n <- -sqrt(-dv_n) T_n: T_out = diag(dv) T, what pass 2 takes as T_in
#include "sgp_common.hpp"
#include "sgp_stream.hpp"
#include "sgp_dense.hpp"
#include "sgp_ctx.hpp"
#include "sgp_lik.hpp"
#include "sgp_sgpmc_lik.hpp"

namespace sgp {

// One workgroup per ASM_ROWS rows.  Phase 1: wave w owns rows [64 w, 64 w + 64), four at a time; a lane reads 16 bytes of each row per
// step of 128 columns, v comes from LDS, the two sums of a row are closed by the wave butterfly.  Phase 2: one thread per row runs the
// likelihood.  The per-workgroup partials [ell | ds2 | dv] are added up by last_block_sums (sgp_common.hpp): in index order, by the
// workgroup that draws the last ticket.
// LDS (dynamic, one array): v (Mp) | t.v of the rows (256) | |t|^2 of the rows (256) | block_sum256's 4 words | the "I am last" word.
// The rows are a_n = scale T_n and k(x_n, x_n) = knn: (sf2, sf2) for the unit-amplitude T of a stationary kernel, (1, kdiag + white) for
// the full-amplitude T of a composite one (sgp_sgpmc_comp.hip), which also brings the optional mean function `mean` (N, added to mu)
// and the optional outputs mu_out / var_out (N; var as it is formed, not floored).  y == nullptr: the moments only -- no likelihood,
// dmu = dv = 0 and zero sums (dmu / dv may be null then).
__global__ __launch_bounds__(256) void sgpmc_lik_rows_kernel(const double* __restrict__ T, const double* __restrict__ y,
                                                             const double* __restrict__ mean, const double* __restrict__ v, int64_t N,
                                                             int M, int Mp, double scale, double knn, double s2, int lik, GHTable gh,
                                                             double* __restrict__ dmu, double* __restrict__ dv,
                                                             double* __restrict__ mu_out, double* __restrict__ var_out,
                                                             double* __restrict__ dmu_pad, double* __restrict__ dv_pad, double* part,
                                                             int* __restrict__ counter, double* __restrict__ out) {
  extern __shared__ double lds[];
  double* vsh = lds;
  double* tv = lds + Mp;
  double* tt = tv + ASM_ROWS;
  double* red = tt + ASM_ROWS;
  double* last = red + 4;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int c = tid; c < Mp; c += 256) vsh[c] = c < M ? v[c] : 0.0;
  __syncthreads();
  const int64_t rbase = (int64_t)blockIdx.x * ASM_ROWS;
  for (int rr = 0; rr < 64; rr += 4) {
    const double* t0 = T + (size_t)(rbase + wv * 64 + rr) * Mp;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
    for (int c = 2 * lane; c < Mp; c += 128) {
      const d2 vv = *reinterpret_cast<const d2*>(vsh + c);
      const d2 a0 = *reinterpret_cast<const d2*>(t0 + c);
      const d2 a1 = *reinterpret_cast<const d2*>(t0 + (size_t)Mp + c);
      const d2 a2 = *reinterpret_cast<const d2*>(t0 + 2 * (size_t)Mp + c);
      const d2 a3 = *reinterpret_cast<const d2*>(t0 + 3 * (size_t)Mp + c);
      m0 = fma(a0.y, vv.y, fma(a0.x, vv.x, m0)); q0 = fma(a0.y, a0.y, fma(a0.x, a0.x, q0));
      m1 = fma(a1.y, vv.y, fma(a1.x, vv.x, m1)); q1 = fma(a1.y, a1.y, fma(a1.x, a1.x, q1));
      m2 = fma(a2.y, vv.y, fma(a2.x, vv.x, m2)); q2 = fma(a2.y, a2.y, fma(a2.x, a2.x, q2));
      m3 = fma(a3.y, vv.y, fma(a3.x, vv.x, m3)); q3 = fma(a3.y, a3.y, fma(a3.x, a3.x, q3));
    }
    m0 = wave_sum(m0); m1 = wave_sum(m1); m2 = wave_sum(m2); m3 = wave_sum(m3);
    q0 = wave_sum(q0); q1 = wave_sum(q1); q2 = wave_sum(q2); q3 = wave_sum(q3);
    if (lane == 0) {
      const int r = wv * 64 + rr;
      tv[r] = m0; tv[r + 1] = m1; tv[r + 2] = m2; tv[r + 3] = m3;
      tt[r] = q0; tt[r + 1] = q1; tt[r + 2] = q2; tt[r + 3] = q3;
    }
  }
  __syncthreads();
  const int64_t n = rbase + tid;
  double ell = 0.0, gm = 0.0, gv = 0.0, gs = 0.0;
  if (n < N) {
    double mu = scale * tv[tid];
    if (mean) mu += mean[n];
    const double var = knn - (scale * scale) * tt[tid];
    if (mu_out) mu_out[n] = mu;
    if (var_out) var_out[n] = var;
    if (y) {
      lik_eval_floored(lik, y[n], mu, var, knn * 0x1p-40, s2, gh, ell, gm, gv, gs);
      // dv <= 0 for these likelihoods, but a quadrature whose nodes are all saturated returns rounding noise of either sign around 0
      // (1e-17 of dmu): a positive one is 0 here, so that sqrt(-dv) below is real.  (A NaN stays a NaN.)
      if (gv > 0.0) gv = 0.0;
    }
    if (dmu) dmu[n] = gm;
    if (dv) dv[n] = gv;
  }
  dmu_pad[n] = gm;
  dv_pad[n] = gv;
  double s[3];
  s[0] = block_sum256(ell, red);
  s[1] = block_sum256(gs, red);
  s[2] = block_sum256(gv, red);
  if (!last_block_sums(s, part, counter, red, last)) return;
  if (tid == 0) {
    out[0] = s[0];
    out[1] = s[1];
    out[2] = s[2];
  }
}

// the same outputs for an empty shard (of every row pass that writes [sum ell | sum ds2 | sum dv])
__global__ void sgpmc_lik_empty_kernel(double* __restrict__ out) {
  if (threadIdx.x < SGP_SGPMC_LIK_OUT_LEN) out[threadIdx.x] = 0.0;
}

// T_n <- sign sqrt(-dv_n) T_n in place, 16 bytes per thread and step; a workgroup takes 16 rows at a time.  The padding (rows >= N,
// columns >= M) is written as zeros whatever dv holds, so a non-finite dv never reaches it.
constexpr int SCALE_ROWS = 16;
constexpr int SCALE_MAX_GROUPS = 4096;  // workgroups of a launch (16 per CU); beyond 65536 rows each takes several 16-row groups
__global__ __launch_bounds__(256) void sgpmc_lik_scale_kernel(double* __restrict__ T, const double* __restrict__ dv_pad, int64_t N,
                                                              int64_t Npad, int M, int Mp, double sign) {
  __shared__ double s[SCALE_ROWS];
  const int half = Mp >> 1, per = SCALE_ROWS * half;
  for (int64_t g = blockIdx.x; g < Npad / SCALE_ROWS; g += gridDim.x) {
    const int64_t r0 = g * SCALE_ROWS;
    __syncthreads();
    if (threadIdx.x < SCALE_ROWS) s[threadIdx.x] = sign * sqrt(-dv_pad[r0 + threadIdx.x]);
    __syncthreads();
    d2* base = reinterpret_cast<d2*>(T + (size_t)r0 * Mp);
    for (int li = threadIdx.x; li < per; li += 256) {
      const int r = li / half, c = 2 * (li - r * half);
      const bool row_live = r0 + r < N;
      const d2 t = base[li];
      d2 o;
      o.x = (row_live && c < M) ? s[r] * t.x : 0.0;
      o.y = (row_live && c + 1 < M) ? s[r] * t.y : 0.0;
      base[li] = o;
    }
  }
}

void sgpmc_lik_rows_launch(const double* T, const double* y, const double* mean, const double* v, int64_t N, int64_t Npad, int M, int Mp,
                           double scale, double knn, double s2, int lik, double* dmu, double* dv, double* mu_out, double* var_out,
                           double* dmu_pad, double* dv_pad, double* part, int* counter, double* out, hipStream_t st) {
  static const GHTable gh = make_gh();
  const size_t lds = ((size_t)Mp + 2 * ASM_ROWS + 8) * sizeof(double);
  sgpmc_lik_rows_kernel<<<(unsigned)(Npad / ASM_ROWS), 256, lds, st>>>(T, y, mean, v, N, M, Mp, scale, knn, s2, lik, gh, dmu, dv, mu_out,
                                                                      var_out, dmu_pad, dv_pad, part, counter, out);
}
void sgpmc_lik_empty_launch(double* out, hipStream_t st) { sgpmc_lik_empty_kernel<<<1, 64, 0, st>>>(out); }
void sgpmc_lik_scale_launch(double* T, const double* dv_pad, int64_t N, int64_t Npad, int M, int Mp, double sign, hipStream_t st) {
  const int64_t groups = Npad / SCALE_ROWS;
  const int sgrid = (int)(groups < SCALE_MAX_GROUPS ? groups : SCALE_MAX_GROUPS);
  sgpmc_lik_scale_kernel<<<sgrid, 256, 0, st>>>(T, dv_pad, N, Npad, M, Mp, sign);
}

struct LikRowsWs {
  WhRowsWs wh;
  double *dmu_pad, *dv_pad, *part, *scratch;
  int* counter;
  size_t bytes;
};
static LikRowsWs carve_lik_rows(void* ws, const StreamPlan& p) {
  LikRowsWs w;
  w.wh = carve_wh_rows(ws, p, true);
  Carver c(ws ? static_cast<char*>(ws) + w.wh.bytes : nullptr);
  const size_t rows = (size_t)(p.Npad > 0 ? p.Npad : 1);
  w.dmu_pad = c.take<double>(rows);
  w.dv_pad = c.take<double>(rows);
  w.part = c.take<double>(3 * (rows / ASM_ROWS + 1));
  w.scratch = c.take<double>(2);
  w.counter = c.take<int>(1);
  w.bytes = w.wh.bytes + c.used();
  return w;
}

}  // namespace sgp

using namespace sgp;

extern "C" size_t sgp_sgpmc_lik_rows_workspace_bytes(int64_t N, int M, int d) {
  if (!stream_shape_ok(N, M, d)) return 0;
  StreamPlan p;
  if (!rows_plan(N, M, d, p)) return 0;
  return carve_lik_rows(nullptr, p).bytes;
}

extern "C" int sgp_sgpmc_lik_rows(const double* X, int64_t ldx, const double* y, const double* Z, int64_t ldz, const double* inv_ls,
                                  double sf2, double s2, const double* v, int64_t N, int M, int d, int kernel_id, int likelihood_id,
                                  const double* kuu_linv, int want_adjoints, double* out, double* G, double* g, double* dmu, double* dv,
                                  double* T_out, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  const Ctx& cx = cur_ctx();
  if (likelihood_id < 0 || likelihood_id > LIK_ID_MAX) return SGP_ERR_ARG;
  if (likelihood_id == SGP_LIK_GAUSSIAN && !(s2 > 0.0)) return SGP_ERR_ARG;
  if (want_adjoints && (!G || !g)) return SGP_ERR_ARG;
  if (N > 0 && (!dmu || !dv)) return SGP_ERR_ARG;
  if (const int bad = check_stream_args({Z, inv_ls, kuu_linv, v, out, T_out}, X, ldx, y, ldz, N, M, d, kernel_id, false)) return bad;
  StreamPlan p;
  if (!rows_plan(N, M, d, p)) return SGP_ERR_WORKSPACE;
  LikRowsWs w = carve_lik_rows(ws, p);
  if (!ws || ws_bytes < w.bytes) return SGP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const FwdWs& f = w.wh.f;
  if (p.Npad == 0) {
    sgpmc_lik_empty_launch(out, st);
    if (want_adjoints) {
      fill_zero(G, (size_t)M * M, st);
      fill_zero(g, (size_t)M, st);
    }
    return check_launch();
  }
  stream_rows_start(p, kernel_id, make_kern_args(inv_ls, sf2, d), X, ldx, y, Z, ldz, N, M, kuu_linv, w.wh, T_out, st);
  zero_ints(w.counter, 1, st);
  sgpmc_lik_rows_launch(T_out, y, nullptr, v, N, p.Npad, M, p.Mp, sf2, sf2, s2, likelihood_id, dmu, dv, nullptr, nullptr, w.dmu_pad,
                        w.dv_pad, w.part, w.counter, out, st);
  if (!want_adjoints) return check_launch();
  // g = sf2 T^T dmu: the partials and the reduction of K'^T y (yy and kappa of that reduction go to scratch)
  launch_tpart(T_out, w.dmu_pad, 0, p.Npad, p.Mp, f.bpart, st);
  reduce_bparts(p, f.bpart, f.btmp, f.yypart, 1, sf2, N, M, g, w.scratch, w.scratch + 1, st);
  sgpmc_lik_scale_launch(T_out, w.dv_pad, N, p.Npad, M, p.Mp, 1.0, st);
  launch_syrk(cx, T_out, p.Mp, p.Npad / NB, split_map(p.taper, p.Npad / NB, p.nsplit), p.ntiles, p.nsplit, 0, f.slab, st);
  reduce_slabs(p, f.slab, p.nsplit, M, -(sf2 * sf2), G, st);
  sgpmc_lik_scale_launch(T_out, w.dv_pad, N, p.Npad, M, p.Mp, -1.0, st);
  return check_launch();
}
