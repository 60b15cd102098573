// The M x M tail of SGPMC (Hensman et al. 2015; the reference's models/sgp_hmc.py:38-43, GPflow's SGPMC with a Gaussian likelihood):
// the joint log-density of the whitened inducing values v and the data given v, from the whitened sufficient statistics
// [W | u | yy | kappa] of pass 1 (include/sgp.h states the density and its adjoints).  Nothing is factored here: L^-1 comes from
// sgp_kuu_factor, so the tail is one elementwise / matrix-vector launch, the sandwich L^-T S' L^-1 (linv_sandwich of sgp_dense.hpp: two
// gemm() calls with triangular masks) and one closing launch -- four launches, two without the adjoints.  Both extern "C" tails are
// sgpmc_tail<LIK> below.
#include "sgp_common.hpp"
#include "sgp_dense.hpp"

namespace sgp {

// Launch 1, two jobs by block range (adjoint_mid_kernel's pattern; every sum in a fixed order):
//  blocks [0, Mp / 16): one wave per row i of the padded layout.
//      wv_i = sum_j W[i][j] v_j,  h_i = (u_i - wv_i) / s2  -> hvec[i]  (0 in the padding)
//      rows4[i] = v_i wv_i   rows4[Mp + i] = v_i u_i   rows4[2 Mp + i] = W[i][i]   rows4[3 Mp + i] = v_i^2   (0 in the padding)
//    with the adjoints also row i of Cw = I - v v^T (M x M, ld M) and, for c >= i, the two mirrored entries
//      S'[i][c] = S'[c][i] = -sym(W)[i][c] / (2 s2) - v_c h_i / 2          (Mp x Mp, ld Mp, 0 in the padding)
//    -- sym(low(v h^T))[r][c] = v_max(r,c) h_min(r,c) / 2 on and off the diagonal, so the wave that owns h_i writes every entry whose
//    smaller index is i and no wave waits for another's h.
//  the next Mp / 64 blocks (adjoints only): t = L^-T v, a block per 64 columns, sixteen waves over the rows, the partial sums added in
//    wave order.  The identity-padded rows of L^-1 meet v's zero padding: t is 0 there.
// LIK (the tail of a non-conjugate likelihood, sgp_sgpmc_lik_tail): W := G and u := g arrive as the adjoints themselves, so h = g, the
// triangle is S' = sym(G) - sym(low(v g^T)), only rows4's v_i^2 is used and no Cw is written; the t blocks are the same.
template <bool LIK>
__global__ __launch_bounds__(1024) void sgpmc_mid_kernel(const double* __restrict__ W, const double* __restrict__ u,
                                                         const double* __restrict__ v, const double* __restrict__ Li, int M, int Mp,
                                                         double s2, int with_adj, double* __restrict__ hvec,
                                                         double* __restrict__ rows4, double* __restrict__ Cw, double* __restrict__ Sp,
                                                         double* __restrict__ t) {
  __shared__ double part[16][64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nR = Mp / 16;
  if (b < nR) {
    const int i = b * 16 + wv;
    const bool live = i < M;
    double s = 0.0;
    if constexpr (!LIK) {
      if (live)
        for (int j = lane; j < M; j += 64) s = fma(W[(int64_t)i * M + j], v[j], s);
      s = wave_sum(s);
    }
    const double vi = live ? v[i] : 0.0;
    double hi;
    if constexpr (LIK) hi = (live && with_adj) ? u[i] : 0.0;  // (a value-only call has neither G nor g)
    else hi = live ? (u[i] - s) / s2 : 0.0;
    if (lane == 0) {
      hvec[i] = hi;
      rows4[i] = vi * s;
      rows4[Mp + i] = (live && !LIK) ? vi * u[i] : 0.0;
      rows4[2 * Mp + i] = (live && !LIK) ? W[(int64_t)i * M + i] : 0.0;
      rows4[3 * Mp + i] = vi * vi;
    }
    if (!with_adj) return;
    if constexpr (!LIK) {
      if (live)
        for (int c = lane; c < M; c += 64) Cw[(int64_t)i * M + c] = (c == i ? 1.0 : 0.0) - vi * v[c];
    }
    const double q = LIK ? 1.0 : -0.5 / s2;
    for (int c = i + lane; c < Mp; c += 64) {
      double val = 0.0;
      if (live && c < M) {
        const double w = 0.5 * (W[(int64_t)i * M + c] + W[(int64_t)c * M + i]);
        val = fma(q, w, -0.5 * v[c] * hi);
      }
      Sp[(int64_t)i * Mp + c] = val;
      Sp[(int64_t)c * Mp + i] = val;
    }
    return;
  }
  {
    const int col = (b - nR) * 64 + lane;
    double s0 = 0.0, s1 = 0.0, s2_ = 0.0, s3 = 0.0;
    int j = wv;
    for (; j + 48 < M; j += 64) {
      s0 = fma(Li[(int64_t)j * Mp + col], v[j], s0);
      s1 = fma(Li[(int64_t)(j + 16) * Mp + col], v[j + 16], s1);
      s2_ = fma(Li[(int64_t)(j + 32) * Mp + col], v[j + 32], s2_);
      s3 = fma(Li[(int64_t)(j + 48) * Mp + col], v[j + 48], s3);
    }
    for (; j < M; j += 16) s0 = fma(Li[(int64_t)j * Mp + col], v[j], s0);
    part[wv][lane] = (s0 + s1) + (s2_ + s3);
    __syncthreads();
    if (wv == 0) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) acc += part[k][lane];
      t[col] = acc;
    }
  }
}

// The closing launch: blocks [0, nA) (adjoints only) write Kuubar = sym(R) cropped to M x M (ld M), R = L^-T S' L^-1 in the padded layout;
// block 0 of them also bbar = t / s2 and vbar = h - v.  The last block adds the four row arrays up, each in one fixed order, and writes out.
// LIK: yy points at the row pass's [sum ell | d sum ell / d s2 | sum dv] and the data term is its first entry; s2 = 1, so bbar = t.
template <bool LIK>
__global__ __launch_bounds__(256) void sgpmc_out_kernel(const double* __restrict__ R, const double* __restrict__ t,
                                                        const double* __restrict__ hvec, const double* __restrict__ v,
                                                        const double* __restrict__ rows4, const double* __restrict__ yy,
                                                        const double* __restrict__ kappa, int M, int Mp, double s2, double Nd, int nA,
                                                        double* __restrict__ Kuubar, double* __restrict__ bbar,
                                                        double* __restrict__ vbar, double* __restrict__ out) {
  if ((int)blockIdx.x == nA) {
    __shared__ double red[4];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int i = threadIdx.x; i < Mp; i += 256) {
      a0 += rows4[i];
      a1 += rows4[Mp + i];
      a2 += rows4[2 * Mp + i];
      a3 += rows4[3 * Mp + i];
    }
    const double vWv = block_sum256(a0, red);
    const double vu = block_sum256(a1, red);
    const double trW = block_sum256(a2, red);
    const double vv = block_sum256(a3, red);
    if (threadIdx.x != 0) return;
    const double LOG2PI = 1.8378770664093453;
    if constexpr (LIK) {
      const double prior = -0.5 * vv - 0.5 * (double)M * LOG2PI;
      out[SGP_SGPMC_OUT_F] = yy[0] + prior;
      out[SGP_SGPMC_OUT_DATA] = yy[0];
      out[SGP_SGPMC_OUT_PRIOR] = prior;
      out[SGP_SGPMC_OUT_S2BAR] = yy[1];
      out[SGP_SGPMC_OUT_KAPPABAR] = Nd > 0.0 ? yy[2] / Nd : 0.0;
      return;
    }
    const double Q = *yy - 2.0 * vu + vWv + *kappa - trW;
    const double data = -0.5 * Nd * (LOG2PI + log(s2)) - Q / (2.0 * s2);
    const double prior = -0.5 * vv - 0.5 * (double)M * LOG2PI;
    out[SGP_SGPMC_OUT_F] = data + prior;
    out[SGP_SGPMC_OUT_DATA] = data;
    out[SGP_SGPMC_OUT_PRIOR] = prior;
    out[SGP_SGPMC_OUT_S2BAR] = -0.5 * Nd / s2 + Q / (2.0 * s2 * s2);
    out[SGP_SGPMC_OUT_KAPPABAR] = -1.0 / (2.0 * s2);
    return;
  }
  const int64_t total = (int64_t)M * M;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)nA * 256) {
    const int r = (int)(e / M), c = (int)(e - (int64_t)r * M);
    Kuubar[e] = 0.5 * (R[(int64_t)r * Mp + c] + R[(int64_t)c * Mp + r]);
  }
  if (blockIdx.x == 0) {
    const double is2 = 1.0 / s2;
    for (int i = threadIdx.x; i < M; i += 256) {
      bbar[i] = t[i] * is2;
      vbar[i] = hvec[i] - v[i];
    }
  }
}

struct SgpmcWs {
  double *Sp, *T, *R, *hvec, *t, *rows4;
  size_t bytes;
};
static SgpmcWs carve_sgpmc(void* ws, int Mp) {
  Carver c(ws);
  SgpmcWs w;
  const size_t mm = (size_t)Mp * Mp;
  w.Sp = c.take<double>(mm);
  w.T = c.take<double>(mm);
  w.R = c.take<double>(mm);
  w.hvec = c.take<double>(Mp);
  w.t = c.take<double>(Mp);
  w.rows4 = c.take<double>((size_t)4 * Mp);
  w.bytes = c.used();
  return w;
}

// Both tails: the shared checks (every SGP_ERR_ARG ahead of SGP_ERR_DIM; a tail's own stand in front of this call), the carve and the
// launches.  (W, u, yy, kappa) are the whitened statistics, or with LIK (G, g, the row pass's three sums, nullptr).
template <bool LIK>
static int sgpmc_tail(const double* W, const double* u, const double* yy, const double* kappa, const double* v, double s2, int64_t N, int M,
                      int with_adjoints, double* out, double* vbar, double* Cw, double* bbar, double* Kuubar, const double* kuu_linv,
                      void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!yy || !v || !out || M <= 0 || N < 0) return SGP_ERR_ARG;
  if (with_adjoints && (!vbar || !bbar || !Kuubar || !kuu_linv)) return SGP_ERR_ARG;
  if (M > SGP_MAX_INDUCING) return SGP_ERR_DIM;
  const int Mp = padded_m(M);
  SgpmcWs w = carve_sgpmc(ws, Mp);
  if (!ws || ws_bytes < w.bytes) return SGP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int adj = with_adjoints ? 1 : 0;
  sgpmc_mid_kernel<LIK><<<Mp / 16 + (adj ? Mp / 64 : 0), 1024, 0, st>>>(W, u, v, kuu_linv, M, Mp, s2, adj, w.hvec, w.rows4, Cw, w.Sp, w.t);
  const int nA = adj ? linv_sandwich(w.Sp, kuu_linv, M, Mp, w.T, w.R, st) : 0;
  sgpmc_out_kernel<LIK><<<nA + 1, 256, 0, st>>>(w.R, w.t, w.hvec, v, w.rows4, yy, kappa, M, Mp, s2, (double)N, nA, Kuubar, bbar, vbar, out);
  return check_launch();
}

}  // namespace sgp

using namespace sgp;

extern "C" size_t sgp_sgpmc_workspace_bytes(int M) {
  if (M <= 0 || M > SGP_MAX_INDUCING) return 0;
  return carve_sgpmc(nullptr, padded_m(M)).bytes;
}

extern "C" int sgp_sgpmc_from_whitened_stats(const double* W, const double* u, const double* yy, const double* kappa, const double* v,
                                             double s2, int64_t N, int M, int with_adjoints, double* out, double* vbar, double* Cw,
                                             double* bbar, double* Kuubar, const double* kuu_linv, void* ws, size_t ws_bytes,
                                             sgp_stream_t stream) {
  if (!W || !u || !kappa || !(s2 > 0.0) || (with_adjoints && !Cw)) return SGP_ERR_ARG;
  return sgpmc_tail<false>(W, u, yy, kappa, v, s2, N, M, with_adjoints, out, vbar, Cw, bbar, Kuubar, kuu_linv, ws, ws_bytes, stream);
}

// The tail behind sgp_sgpmc_lik_rows: the same four launches on (G, g) in place of (W, u), with s2 = 1.
extern "C" size_t sgp_sgpmc_lik_workspace_bytes(int M) { return sgp_sgpmc_workspace_bytes(M); }

extern "C" int sgp_sgpmc_lik_tail(const double* rows_out, const double* G, const double* g, const double* v, int64_t N, int M,
                                  int with_adjoints, double* out, double* vbar, double* bbar, double* Kuubar, const double* kuu_linv,
                                  void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (with_adjoints && (!G || !g)) return SGP_ERR_ARG;
  return sgpmc_tail<true>(G, g, rows_out, nullptr, v, 1.0, N, M, with_adjoints, out, vbar, nullptr, bbar, Kuubar, kuu_linv, ws, ws_bytes,
                          stream);
}
