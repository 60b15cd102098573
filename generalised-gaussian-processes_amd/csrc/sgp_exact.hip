// The exact GP marginal likelihood and its gradient (reference models/gpr_hmc.py:43-59: pm.gp.Marginal with noise sig_n over
// sig_f^2 ExpQuad(ls)), and the exact posterior predictive.
//
//   A = K(X, X) + s2 I ; L = chol(A) ; u = L^-1 y ; alpha = L^-T u ; G = alpha alpha^T - A^-1
//   F        = -1/2 u.u - sum log L_ii - N/2 log 2 pi
//   dF/dls_q = 1/2 sum_ij G_ij dK_ij/dls_q ; dF/dsf2 = 1/2 sum_ij G_ij k'_ij ; dF/ds2 = 1/2 (alpha.alpha - tr A^-1)
//
// A is assembled by sgp_kuu's kernel (X in place of Z, jitter = s2: WhiteNoise(sig_n) adds sig_n^2 to the diagonal and nothing
// else) and factored by the sgp_kuu_factor_ex chain, which forms L^-1 and tr(A^-1) inside its launches and applies the context's
// conditioning gate.  The gradient never writes A^-1: exact_grad_kernel forms each 64 x 64 lower-triangle tile of L^-T L^-1 on the
// fp64 matrix cores and folds it into the d + 1 sums in its epilogue.
#include "sgp_dense.hpp"
#include "sgp_ctx.hpp"

namespace sgp {

static KernArgs make_ka_e(const double* inv_ls, double sf2, int d) {
  KernArgs ka;
  for (int j = 0; j < SGP_MAX_DIM; ++j) ka.inv_ls[j] = (inv_ls && j < d) ? inv_ls[j] : 0.0;
  ka.sf2 = sf2;
  ka.d = d;
  return ka;
}
static int grid_for_e(int64_t total, int cap = 2048) {
  int64_t g = (total + 255) / 256;
  if (g < 1) g = 1;
  return (int)(g < cap ? g : cap);
}

constexpr int ET = 64;  // tile edge of the gradient kernel

static int exact_np(int64_t N) { return padded_m((int)N); }
static int exact_tiles(int64_t N) {
  const int nb = (int)((N + ET - 1) / ET);
  return nb * (nb + 1) / 2;
}

// yp <- y zero-padded to Np
__global__ __launch_bounds__(256) void exact_pad_kernel(const double* __restrict__ y, int N, int Np, double* __restrict__ yp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < Np) yp[i] = i < N ? y[i] : 0.0;
}

// One workgroup, after u = L^-1 y and alpha = L^-T u (two gemv launches of sgp_dense.hip): the scalars of the evaluation.
//   out = [F, y^T A^-1 y = u.u, log|A| = -2 sum log (L^-1)_ii, tr A^-1] ; g_s2 = (alpha.alpha - tr A^-1) / 2 (when wanted)
// Fixed thread <-> index mapping and block_sum256's fixed tree: the same bits on every call.
__global__ __launch_bounds__(256) void exact_alpha_kernel(const double* __restrict__ Linv, int Np, int N, const double* __restrict__ u,
                                                          const double* __restrict__ alpha, const double* __restrict__ trace,
                                                          double* __restrict__ out, double* __restrict__ g_s2) {
  __shared__ double red[4];
  double uu = 0.0, aa = 0.0, ld = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) {
    uu = fma(u[i], u[i], uu);
    aa = fma(alpha[i], alpha[i], aa);
    ld += log(Linv[(int64_t)i * Np + i]);
  }
  uu = block_sum256(uu, red);
  aa = block_sum256(aa, red);
  ld = block_sum256(ld, red);
  if (threadIdx.x == 0) {
    const double logdet = -2.0 * ld;
    const double tr = trace[0];
    out[0] = -0.5 * uu - 0.5 * logdet - 0.5 * (double)N * 1.8378770664093453;  // log 2 pi
    out[1] = uu;
    out[2] = logdet;
    out[3] = tr;
    if (g_s2) *g_s2 = 0.5 * (aa - tr);
  }
}

// The hot path.  Workgroup <-> lower-triangle tile (I, J), I >= J, of A^-1 = L^-T L^-1 (64 x 64); wave w <-> the 32 x 32 quadrant
// (w >> 1, w & 1), four 16 x 16 v_mfma_f64_16x16x4_f64 accumulators.  (A^-1)_ij = sum_{k >= max(i, j)} (L^-1)_ki (L^-1)_kj: the k loop
// starts at the quadrant's first row -- the zeros of L^-1 above its diagonal are never multiplied -- and ends at N rounded up to 4
// (rows N .. Np of the padded factor are identity rows, zero in the columns < N).  Epilogue: G = alpha_i alpha_j - tile, K'_ij and the
// squared scaled differences recomputed from X (staged in LDS) with kprofile_grad as kuu_bwd_kernel does, and
//   part[tile][q] = sum w G h (x~_iq - x~_jq)^2  (q < d) ,  part[tile][d] = sum w G k'
// with w = 2 below the diagonal, 1 on it, 0 above (a diagonal tile's upper quadrant is skipped whole).  Fixed order throughout.
template <int KID>
__global__ __launch_bounds__(256) void exact_grad_kernel(const double* __restrict__ Linv, int Np, int N, int kend,
                                                         const double* __restrict__ X, int64_t ldx, KernArgs ka,
                                                         const double* __restrict__ alpha, double* __restrict__ part) {
  __shared__ double xi[ET][SGP_MAX_DIM + 1], xj[ET][SGP_MAX_DIM + 1];
  __shared__ double ai[ET], aj[ET];
  __shared__ double red[4][SGP_MAX_DIM + 1];
  const int t = blockIdx.x;
  int I = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  const int d = ka.d;
  for (int e = threadIdx.x; e < ET * d; e += 256) {
    const int r = e / d, q = e - r * d;
    const int gi = I * ET + r, gj = J * ET + r;
    xi[r][q] = gi < N ? X[(int64_t)gi * ldx + q] : 0.0;
    xj[r][q] = gj < N ? X[(int64_t)gj * ldx + q] : 0.0;
  }
  if (threadIdx.x < ET) {
    const int gi = I * ET + threadIdx.x, gj = J * ET + threadIdx.x;
    ai[threadIdx.x] = gi < N ? alpha[gi] : 0.0;
    aj[threadIdx.x] = gj < N ? alpha[gj] : 0.0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const bool diag = I == J;
  const bool active = !(diag && wc > wr);
  double s[SGP_MAX_DIM];
#pragma unroll
  for (int q = 0; q < SGP_MAX_DIM; ++q) s[q] = 0.0;
  double sk = 0.0;
  if (active) {
    const int i0 = I * ET + wr * 32, j0 = J * ET + wc * 32;
    const int lr = lane & 15, lk = lane >> 4;
    d4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc01 = acc00, acc10 = acc00, acc11 = acc00;
    const int k0 = i0 > j0 ? i0 : j0;
    const double* p = Linv + (int64_t)(k0 + lk) * Np;
    int k = k0;
    for (; k + 16 <= kend; k += 16) {
      double a0[4], a1[4], b0[4], b1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double* r = p + (int64_t)(4 * u) * Np;
        a0[u] = r[i0 + lr];
        a1[u] = r[i0 + 16 + lr];
        b0[u] = r[j0 + lr];
        b1[u] = r[j0 + 16 + lr];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc00 = mfma16(a0[u], b0[u], acc00);
        acc01 = mfma16(a0[u], b1[u], acc01);
        acc10 = mfma16(a1[u], b0[u], acc10);
        acc11 = mfma16(a1[u], b1[u], acc11);
      }
      p += (int64_t)16 * Np;
    }
    for (; k < kend; k += 4) {
      const double a0 = p[i0 + lr], a1 = p[i0 + 16 + lr], b0 = p[j0 + lr], b1 = p[j0 + 16 + lr];
      acc00 = mfma16(a0, b0, acc00);
      acc01 = mfma16(a0, b1, acc01);
      acc10 = mfma16(a1, b0, acc10);
      acc11 = mfma16(a1, b1, acc11);
      p += (int64_t)4 * Np;
    }
    // epilogue: element r of an accumulator is row (lane >> 4) + 4 r, column lane & 15 of its 16 x 16 block
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      const int bi = blk >> 1, bj = blk & 1;
      const d4 acc = blk == 0 ? acc00 : blk == 1 ? acc01 : blk == 2 ? acc10 : acc11;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int li = wr * 32 + bi * 16 + lk + 4 * r, lj = wc * 32 + bj * 16 + lr;  // within the 64 x 64 tile
        const int gi = I * ET + li, gj = J * ET + lj;
        double w = diag ? (li > lj ? 2.0 : (li == lj ? 1.0 : 0.0)) : 2.0;
        if (gi >= N || gj >= N) w = 0.0;
        const double g = w * fma(ai[li], aj[lj], -acc[r]);
        double r2 = 0.0;
#pragma unroll
        for (int q = 0; q < SGP_MAX_DIM; ++q) {
          if (q < d) {
            const double df = (xi[li][q] - xj[lj][q]) * ka.inv_ls[q];
            r2 = fma(df, df, r2);
          }
        }
        double kp, hp;
        kprofile_grad<KID>(r2, kp, hp);
        sk = fma(g, kp, sk);
        const double e = g * hp;
#pragma unroll
        for (int q = 0; q < SGP_MAX_DIM; ++q) {
          if (q < d) {
            const double df = (xi[li][q] - xj[lj][q]) * ka.inv_ls[q];
            s[q] = fma(e * df, df, s[q]);
          }
        }
      }
    }
  }
  sk = wave_sum(sk);
  if (lane == 0) red[wave][d] = sk;
#pragma unroll
  for (int q = 0; q < SGP_MAX_DIM; ++q) {
    if (q < d) {
      const double a = wave_sum(s[q]);
      if (lane == 0) red[wave][q] = a;
    }
  }
  __syncthreads();
  if (threadIdx.x <= d) {
    const int q = threadIdx.x;
    part[(size_t)t * (d + 1) + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
  }
}

// One workgroup: the tiles' partials added in a fixed order (wave w takes sums w, w + 4, ..., lanes stride over the tiles), then
// g_ls[q] = 1/2 sum w G dK/dls_q = -sf2 inv_ls_q part_q  and  g_sf2 = part_d / 2.
__global__ __launch_bounds__(256) void exact_grad_reduce_kernel(const double* __restrict__ part, int ntile, KernArgs ka,
                                                                double* __restrict__ g_ls, double* __restrict__ g_sf2) {
  const int d = ka.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = wave; q <= d; q += 4) {
    double s = 0.0;
    for (int m = lane; m < ntile; m += 64) s += part[(size_t)m * (d + 1) + q];
    s = wave_sum(s);
    if (lane == 0) {
      if (q == d) *g_sf2 = 0.5 * s;
      else g_ls[q] = -ka.sf2 * ka.inv_ls[q] * s;
    }
  }
}

// ---- predictive -----------------------------------------------------------------------------------------------------------------
// Kxs[n][t] = sf2 k'(x_n, xs_t) for n < N, t < T (zero in the padding); Np x Tp, ld Tp
template <int KID>
__global__ __launch_bounds__(256) void exact_kxs_kernel(const double* __restrict__ X, int64_t ldx, const double* __restrict__ Xs,
                                                        int64_t ldxs, KernArgs ka, int N, int Np, int T, int Tp, double* __restrict__ K) {
  const int64_t total = (int64_t)Np * Tp;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int n = (int)(e / Tp), t = (int)(e - (int64_t)n * Tp);
    double v = 0.0;
    if (n < N && t < T) {
      double r2 = 0.0;
      for (int q = 0; q < ka.d; ++q) {
        const double df = (X[n * ldx + q] - Xs[t * ldxs + q]) * ka.inv_ls[q];
        r2 = fma(df, df, r2);
      }
      v = ka.sf2 * kprofile<KID>(r2);
    }
    K[e] = v;
  }
}
// mean[t] = sum_n Kxs[n][t] alpha[n] ; var[t] = sf2 - sum_n V[n][t]^2 (+ s2)
__global__ __launch_bounds__(256) void exact_pred_cols_kernel(const double* __restrict__ K, const double* __restrict__ V,
                                                              const double* __restrict__ alpha, int Np, int Tp, int T, double sf2,
                                                              double s2, int pred_noise, double* __restrict__ mean,
                                                              double* __restrict__ var) {
  __shared__ double pm[4][64], pv[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
  double sm = 0.0, sv = 0.0;
  for (int n = w; n < Np; n += 4) {
    const double v = V[(int64_t)n * Tp + col];
    sm = fma(K[(int64_t)n * Tp + col], alpha[n], sm);
    sv = fma(v, v, sv);
  }
  pm[w][threadIdx.x & 63] = sm;
  pv[w][threadIdx.x & 63] = sv;
  __syncthreads();
  if (w == 0 && col < T) {
    const int l = threadIdx.x;
    mean[col] = (pm[0][l] + pm[1][l]) + (pm[2][l] + pm[3][l]);
    if (var) var[col] = sf2 - ((pv[0][l] + pv[1][l]) + (pv[2][l] + pv[3][l])) + (pred_noise ? s2 : 0.0);
  }
}
// cov[a][b] = k(xs_a, xs_b) - (V^T V)[a][b] (symmetrised) (+ s2 on the diagonal); cov has leading dimension ldc
template <int KID>
__global__ __launch_bounds__(256) void exact_pred_cov_kernel(const double* __restrict__ Xs, int64_t ldxs, KernArgs ka,
                                                             const double* __restrict__ VtV, int Tp, int T, int64_t ldc, double s2,
                                                             int pred_noise, double* __restrict__ cov) {
  const int64_t total = (int64_t)T * T;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int a = (int)(e / T), b = (int)(e - (int64_t)a * T);
    double r2 = 0.0;
    for (int q = 0; q < ka.d; ++q) {
      const double df = (Xs[a * ldxs + q] - Xs[b * ldxs + q]) * ka.inv_ls[q];
      r2 = fma(df, df, r2);
    }
    const int64_t p = (int64_t)a * Tp + b, pt = (int64_t)b * Tp + a;
    double v = ka.sf2 * kprofile<KID>(r2) - 0.5 * (VtV[p] + VtV[pt]);
    if (a == b && pred_noise) v += s2;
    cov[(int64_t)a * ldc + b] = v;
  }
}

}  // namespace sgp

using namespace sgp;

// argument checks shared by the value and the workspace query; SGP_OK or the status, before anything is enqueued
static int exact_check(int64_t N, int d, int kernel_id) {
  if (N <= 0 || d <= 0) return SGP_ERR_ARG;
  if (kernel_id < 0 || kernel_id > SGP_KERNEL_MATERN52) return SGP_ERR_ARG;  // composite kernels: out of scope
  if (N > SGP_MAX_INDUCING || d > SGP_MAX_DIM) return SGP_ERR_DIM;
  return SGP_OK;
}

struct ExactWs {
  double *A, *Linv, *yp, *u, *alpha, *trace, *part;
  void* fws;
  size_t fws_bytes, bytes;
};
static ExactWs carve_exact(void* base, int64_t N, int d) {
  const size_t Np = exact_np(N);
  Carver c(base);
  ExactWs w;
  w.A = c.take<double>((size_t)N * N);
  w.Linv = c.take<double>(Np * Np);
  w.yp = c.take<double>(Np);
  w.u = c.take<double>(Np);
  w.alpha = c.take<double>(Np);
  w.trace = c.take<double>(sgp_kuu_inverse_trace_len());
  w.part = c.take<double>((size_t)exact_tiles(N) * (d + 1));
  w.fws_bytes = sgp_kuu_factor_workspace_bytes((int)N);
  w.fws = c.take<char>(w.fws_bytes);
  w.bytes = c.used();
  return w;
}

extern "C" size_t sgp_exact_workspace_bytes(int64_t N, int d, int with_grad) {
  (void)with_grad;  // one size for both modes
  if (exact_check(N, d, 0) != SGP_OK) return 0;
  return carve_exact(nullptr, N, d).bytes;
}
extern "C" size_t sgp_exact_factors_len(int64_t N) {
  if (N <= 0 || N > SGP_MAX_INDUCING) return 0;
  const size_t Np = exact_np(N);
  return Np * Np + Np;
}

extern "C" int sgp_exact_eval(const double* X, int64_t ldx, const double* y, int64_t N, int d, const double* inv_ls, double sf2, double s2,
                              int kernel_id, int with_grad, double* out, double* grads, double* factors, int* info, void* ws,
                              size_t ws_bytes, sgp_stream_t stream) {
  if (!X || !y || !inv_ls || !out || !info || (with_grad && !grads) || ldx < d) return SGP_ERR_ARG;
  const int chk = exact_check(N, d, kernel_id);
  if (chk != SGP_OK) return chk;
  if (!(sf2 > 0.0) || !(s2 >= 0.0)) return SGP_ERR_ARG;
  if (!ws || ws_bytes < sgp_exact_workspace_bytes(N, d, with_grad)) return SGP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)N, Np = exact_np(N);
  ExactWs w = carve_exact(ws, N, d);
  double* Linv = factors ? factors : w.Linv;
  double* alpha = factors ? factors + (size_t)Np * Np : w.alpha;
  // A = K(X, X) + s2 I ; L^-1, tr(A^-1) and the status word (cleared there) from the gated factorization chain
  int rc = sgp_kuu(X, ldx, inv_ls, sf2, s2, n, d, kernel_id, w.A, stream);
  if (rc != SGP_OK) return rc;
  rc = sgp_kuu_factor_ex(w.A, n, Linv, info, w.trace, w.fws, w.fws_bytes, stream);
  if (rc != SGP_OK) return rc;
  exact_pad_kernel<<<(Np + 255) / 256, 256, 0, st>>>(y, n, Np, w.yp);
  gemv(Linv, Np, Np, false, w.yp, w.u, st);   // u = L^-1 y
  gemv(Linv, Np, Np, true, w.u, alpha, st);   // alpha = L^-T u
  const KernArgs ka = make_ka_e(inv_ls, sf2, d);
  exact_alpha_kernel<<<1, 256, 0, st>>>(Linv, Np, n, w.u, alpha, w.trace, out, with_grad ? grads + d + 1 : nullptr);
  if (with_grad) {
    const int ntile = exact_tiles(N);
    const int kend = round_up(n, 4);
    switch (kernel_id) {
      case SGP_KERNEL_RBF: exact_grad_kernel<SGP_KERNEL_RBF><<<ntile, 256, 0, st>>>(Linv, Np, n, kend, X, ldx, ka, alpha, w.part); break;
      case SGP_KERNEL_MATERN32: exact_grad_kernel<SGP_KERNEL_MATERN32><<<ntile, 256, 0, st>>>(Linv, Np, n, kend, X, ldx, ka, alpha, w.part); break;
      default: exact_grad_kernel<SGP_KERNEL_MATERN52><<<ntile, 256, 0, st>>>(Linv, Np, n, kend, X, ldx, ka, alpha, w.part); break;
    }
    exact_grad_reduce_kernel<<<1, 256, 0, st>>>(w.part, ntile, ka, grads, grads + d);
  }
  return check_launch();
}

static int64_t exact_pred_chunk(int64_t T, int want_cov) {
  return want_cov ? round_up64(T, 64) : (T < 16384 ? round_up64(T, 64) : 16384);
}
extern "C" size_t sgp_exact_predict_workspace_bytes(int64_t T, int64_t N, int d, int want_cov) {
  if (T <= 0 || exact_check(N, d, 0) != SGP_OK) return 0;
  if (want_cov && T > 32768) return 0;
  const size_t Np = exact_np(N), Tc = (size_t)exact_pred_chunk(T, want_cov);
  Carver c(nullptr);
  c.take<double>(Np * Tc);
  c.take<double>(Np * Tc);
  if (want_cov) c.take<double>(Tc * Tc);
  return c.used();
}

extern "C" int sgp_exact_predict(const double* Xs, int64_t ldxs, int64_t T, const double* X, int64_t ldx, int64_t N, int d,
                                 const double* inv_ls, double sf2, double s2, const double* factors, int kernel_id, int pred_noise,
                                 double* mean, double* var, double* cov, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!Xs || !X || !inv_ls || !factors || !mean || T <= 0 || ldxs < d || ldx < d) return SGP_ERR_ARG;
  const int chk = exact_check(N, d, kernel_id);
  if (chk != SGP_OK) return chk;
  const int want_cov = cov != nullptr;
  if (want_cov && T > 32768) return SGP_ERR_DIM;  // sgp_predict's full-covariance limit
  if (!ws || ws_bytes < sgp_exact_predict_workspace_bytes(T, N, d, want_cov)) return SGP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)N, Np = exact_np(N);
  const int64_t Tc = exact_pred_chunk(T, want_cov);
  Carver c(ws);
  double* K = c.take<double>((size_t)Np * Tc);
  double* V = c.take<double>((size_t)Np * Tc);
  double* VtV = want_cov ? c.take<double>((size_t)Tc * Tc) : nullptr;
  const double* Linv = factors;
  const double* alpha = factors + (size_t)Np * Np;
  const KernArgs ka = make_ka_e(inv_ls, sf2, d);
  for (int64_t t0 = 0; t0 < T; t0 += Tc) {
    const int Tn = (int)((T - t0) < Tc ? (T - t0) : Tc);
    const int Tp = (int)round_up64(Tn, 64);
    const double* xs = Xs + t0 * ldxs;
    const int g = grid_for_e((int64_t)Np * Tp);
    switch (kernel_id) {  // K_X* chunk, N x T layout, zero in the padding
      case SGP_KERNEL_RBF: exact_kxs_kernel<SGP_KERNEL_RBF><<<g, 256, 0, st>>>(X, ldx, xs, ldxs, ka, n, Np, Tn, Tp, K); break;
      case SGP_KERNEL_MATERN32: exact_kxs_kernel<SGP_KERNEL_MATERN32><<<g, 256, 0, st>>>(X, ldx, xs, ldxs, ka, n, Np, Tn, Tp, K); break;
      default: exact_kxs_kernel<SGP_KERNEL_MATERN52><<<g, 256, 0, st>>>(X, ldx, xs, ldxs, ka, n, Np, Tn, Tp, K); break;
    }
    GemmDesc a;  // V = L^-1 K_X*
    a.A = Linv; a.lda = Np; a.B = K; a.ldb = Tp; a.C = V; a.ldc = Tp;
    a.m = Np; a.n = Tp; a.k = Np; a.khi_mask = 1;
    gemm(a, st);
    exact_pred_cols_kernel<<<Tp / 64, 256, 0, st>>>(K, V, alpha, Np, Tp, Tn, sf2, s2, pred_noise, mean + t0, var ? var + t0 : nullptr);
    if (want_cov) {  // one chunk: Tc covers T
      GemmDesc x;
      x.A = V; x.lda = Tp; x.ta = true; x.B = V; x.ldb = Tp; x.C = VtV; x.ldc = Tp;
      x.m = Tp; x.n = Tp; x.k = Np;
      gemm(x, st);
      const int gc = grid_for_e((int64_t)Tn * Tn);
      switch (kernel_id) {
        case SGP_KERNEL_RBF: exact_pred_cov_kernel<SGP_KERNEL_RBF><<<gc, 256, 0, st>>>(xs, ldxs, ka, VtV, Tp, Tn, T, s2, pred_noise, cov); break;
        case SGP_KERNEL_MATERN32: exact_pred_cov_kernel<SGP_KERNEL_MATERN32><<<gc, 256, 0, st>>>(xs, ldxs, ka, VtV, Tp, Tn, T, s2, pred_noise, cov); break;
        default: exact_pred_cov_kernel<SGP_KERNEL_MATERN52><<<gc, 256, 0, st>>>(xs, ldxs, ka, VtV, Tp, Tn, T, s2, pred_noise, cov); break;
      }
    }
  }
  return check_launch();
}
