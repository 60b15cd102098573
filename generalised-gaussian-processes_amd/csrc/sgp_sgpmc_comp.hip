// SGPMC with a composite kernel, a white-noise term and a mean function (include/sgp.h: sgp_sgpmc_comp_rows, sgp_sgpmc_comp_bwd).
// With K = k(Z, Z) + (J + white) I = L L^T from sgp_kuu / sgp_kuu_factor, the rows a_n^T of T = K_fu L^-T carry the full amplitude:
//   mu_n = a_n.v + mean_n     var_n = kdiag + white - |a_n|^2     ell_n = E_{N(mu_n, var_n)} log p(y_n | f)
// Everything is existing code on a materialised K_fu, one COMP_CHUNK_ROWS chunk at a time:
//   comp_kmatrix, gemm(T = Kc L^-T)            per chunk: T_out holds the whole shard
//   sgpmc_lik_rows_kernel(scale 1, knn)        moments + likelihood, dmu, dv, [sum ell | sum ds2 | sum dv]  (zero_ints ahead of it)
//   -- a value-only / moments-only call ends here --
//   comp_colsum(T, dmu)                        g = T^T dmu, chunks added in order
//   sgpmc_lik_scale_kernel(+1), gemm(-T^T T)   G = -S^T S, S_n = sqrt(-dv_n) a_n^T (dv <= 0: log-concave likelihoods)
//   sgpmc_lik_scale_kernel(-1)                 T_out = diag(dv) T, what sgp_sgpmc_comp_bwd takes as T_in
#include "sgp_common.hpp"
#include "sgp_composite.hpp"
#include "sgp_dense.hpp"
#include "sgp_lik.hpp"
#include "sgp_sgpmc_lik.hpp"
#include "sgp_stream.hpp"

namespace sgp {

struct CompRowsWs {
  double *Kc, *Gp, *gp, *dmu_pad, *dv_pad, *part;
  int* counter;
  size_t bytes;
};
static int64_t comp_rows_chunk(int64_t Npad) { return Npad < COMP_CHUNK_ROWS ? Npad : COMP_CHUNK_ROWS; }
static CompRowsWs carve_comp_rows(void* ws, int64_t Npad, int Mp) {
  CompRowsWs w;
  Carver c(ws);
  w.Kc = c.take<double>((size_t)comp_rows_chunk(Npad) * Mp);
  w.Gp = c.take<double>((size_t)Mp * Mp);
  w.gp = c.take<double>(Mp);
  w.dmu_pad = c.take<double>((size_t)Npad);
  w.dv_pad = c.take<double>((size_t)Npad);
  w.part = c.take<double>(3 * ((size_t)Npad / ASM_ROWS + 1));
  w.counter = c.take<int>(1);
  w.bytes = c.used();
  return w;
}
static bool comp_rows_shape_ok(int64_t N, int M, int d) { return N >= 0 && M > 0 && M <= SGP_MAX_INDUCING && d > 0 && d <= COMP_MAX_DIM; }

}  // namespace sgp

using namespace sgp;

extern "C" size_t sgp_sgpmc_comp_rows_workspace_bytes(int64_t N, int M, int d) {
  if (!comp_rows_shape_ok(N, M, d)) return 0;
  return carve_comp_rows(nullptr, round_up64(N > 0 ? N : 1, ASM_ROWS), padded_m(M)).bytes;
}

extern "C" int sgp_sgpmc_comp_rows(const double* X, int64_t ldx, const double* y, const double* mean, const double* Z, int64_t ldz,
                                   const double* block, double white, double s2, const double* v, int64_t N, int M, int d,
                                   int likelihood_id, const double* kuu_linv, int want_adjoints, double* out, double* G, double* g,
                                   double* dmu, double* dv, double* mu, double* var, double* T_out, void* ws, size_t ws_bytes,
                                   sgp_stream_t stream) {
  if (!Z || !block || !v || !kuu_linv || !out || !T_out) return SGP_ERR_ARG;
  if (N < 0 || M <= 0 || d <= 0 || ldz < d) return SGP_ERR_ARG;
  if (N > 0 && (!X || ldx < d)) return SGP_ERR_ARG;
  if (N > 0 && y && (!dmu || !dv)) return SGP_ERR_ARG;
  if (likelihood_id < 0 || likelihood_id > LIK_ID_MAX) return SGP_ERR_ARG;
  if (likelihood_id == SGP_LIK_GAUSSIAN && !(s2 > 0.0)) return SGP_ERR_ARG;
  if (!(white >= 0.0)) return SGP_ERR_ARG;
  if (want_adjoints && (!G || !g || (N > 0 && !y))) return SGP_ERR_ARG;
  CompSpec cs;
  if (comp_parse(block, d, &cs) != SGP_OK) return SGP_ERR_ARG;  // (d > COMP_MAX_DIM included)
  if (M > SGP_MAX_INDUCING) return SGP_ERR_DIM;
  const int Mp = padded_m(M);
  const int64_t Npad = round_up64(N > 0 ? N : 1, ASM_ROWS);
  CompRowsWs w = carve_comp_rows(ws, Npad, Mp);
  if (!ws || ws_bytes < w.bytes) return SGP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {
    sgpmc_lik_empty_launch(out, st);
    if (want_adjoints) {
      fill_zero(G, (size_t)M * M, st);
      fill_zero(g, (size_t)M, st);
    }
    return check_launch();
  }
  zero_ints(w.counter, 1, st);
  const int64_t Rc = comp_rows_chunk(Npad);
  for (auto [r0, rows] : SuperChunks{Npad, Rc}) {  // r0 < N: Npad - N < ASM_ROWS and r0 is a multiple of it
    const int64_t rn = N - r0 < rows ? N - r0 : rows;
    comp_kmatrix(X + r0 * ldx, ldx, rn, Z, ldz, M, cs, d, rows, Mp, 0.0, w.Kc, st);
    GemmDesc t;  // T = Kc L^-T
    t.A = w.Kc; t.lda = Mp; t.B = kuu_linv; t.ldb = Mp; t.tb = true; t.C = T_out + (size_t)r0 * Mp; t.ldc = Mp;
    t.m = (int)rows; t.n = Mp; t.k = Mp;
    gemm(t, st);
  }
  sgpmc_lik_rows_launch(T_out, y, mean, v, N, Npad, M, Mp, 1.0, cs.kdiag + white, s2, likelihood_id, dmu, dv, mu, var, w.dmu_pad, w.dv_pad,
                        w.part, w.counter, out, st);
  if (!want_adjoints) return check_launch();
  for (auto [r0, rows] : SuperChunks{Npad, Rc})  // g = T^T dmu over the live rows
    comp_colsum(T_out + (size_t)r0 * Mp, Mp, w.dmu_pad + r0, N - r0 < rows ? N - r0 : rows, Mp, r0 > 0, w.gp, st);
  sgpmc_lik_scale_launch(T_out, w.dv_pad, N, Npad, M, Mp, 1.0, st);
  for (auto [r0, rows] : SuperChunks{Npad, Rc}) {  // G = -S^T S
    GemmDesc s;
    s.A = T_out + (size_t)r0 * Mp; s.lda = Mp; s.ta = true; s.B = s.A; s.ldb = Mp; s.C = w.Gp; s.ldc = Mp;
    s.m = Mp; s.n = Mp; s.k = (int)rows; s.alpha = -1.0; s.beta = r0 > 0 ? 1.0 : 0.0;
    gemm(s, st);
  }
  sgpmc_lik_scale_launch(T_out, w.dv_pad, N, Npad, M, Mp, -1.0, st);
  crop_copy(w.Gp, Mp, G, M, M, M, st);
  crop_copy(w.gp, 1, g, 1, M, 1, st);
  return check_launch();
}

extern "C" size_t sgp_sgpmc_comp_bwd_workspace_bytes(int64_t N, int M, int d) {
  if (!comp_rows_shape_ok(N, M, d)) return 0;
  return comp_sgpmc_bwd_workspace_bytes(N, M);
}

extern "C" int sgp_sgpmc_comp_bwd(const double* X, int64_t ldx, const double* dmu, const double* Z, int64_t ldz, const double* block,
                                  const double* T_in, const double* kuu_linv, const double* bbar, int64_t N, int M, int d,
                                  double* g_blk, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!Z || !block || !T_in || !kuu_linv || !bbar || !g_blk) return SGP_ERR_ARG;
  if (N < 0 || M <= 0 || d <= 0 || ldz < d) return SGP_ERR_ARG;
  if (N > 0 && (!X || !dmu || ldx < d)) return SGP_ERR_ARG;
  CompSpec cs;
  if (comp_parse(block, d, &cs) != SGP_OK) return SGP_ERR_ARG;
  if (M > SGP_MAX_INDUCING) return SGP_ERR_DIM;
  return comp_sgpmc_bwd(X, ldx, dmu, Z, ldz, cs, T_in, kuu_linv, bbar, N, M, d, g_blk, ws, ws_bytes, (hipStream_t)stream);
}
