// Multi-class (robust-max) SVGP minibatch bound -- include/sgp.h: sgp_svgp_mc_elbo, sgp_svgp_mc_predict.
//
// [UPSTREAM] GPflow's MultiClass(RobustMax) under SVGP(num_latent_gps = C, whiten = True), as recalled: nothing here could be checked
// against it.  The yardstick is the long-double restatement of the formulas below (tests/svgp_mc_reference.py).
//
// C latent GPs share one kernel, one Z and one minibatch; class c has its own whitened q(u_c) = N(m_c, Ls_c Ls_c^T), Ls_c = tril(LS_c).
//   L = chol(sf2 k'(Z, Z) + J I),  A = L^-1 K_ub,  T_c = Ls_c^T A,  mu_bc = A_b . m_c,  v_bc = sf2 - |A_b|^2 + |T_c,b|^2
//   ell_b = lik_robustmax_pv (sgp_lik.hpp: one variance PER CLASS),  F = mean_b ell_b - sum_c KL(q(u_c) || N(0, I)) / N_total
// Reverse, mubar_c = dmu_c / B, vbar_c = dv_c / B:
//   g_m_c = A mubar_c - m_c / N          g_LS_c = tril(2 A (T_c diag vbar_c)^T) - (Ls_c - diag(1 / diag Ls_c)) / N
//   Abar  = sum_c m_c mubar_c^T + 2 (sum_c Ls_c (T_c diag vbar_c) - A diag(sum_c vbar_c))         direct d/dsf2 = sum_b sum_c vbar_bc
// and from Abar on the chain of sgp_svgp_elbo_batch at S = 1 (sgp_svgp_shared.hpp), once whatever C is.
//
// The launch chain does not depend on C: the class index rides in blockIdx.y, or in GemmDesc::batch2 with A's stride 0.  The C padded
// factors are stored SIDE BY SIDE (LScat: Mp x C Mp, class c at column c Mp), so T_c = Ls_c^T A is a batched product with lda = C Mp and
// sum_c Ls_c (T_c diag vbar_c) is ONE product with k = C Mp over [Ls_0 | .. | Ls_C-1] and the stacked scaled T (T is scaled in place: no
// U_c buffers, no summing launch).  Every sum runs in a fixed order; nothing depends on the workspace's previous contents.
//   mc_prep (C factors, C means, status word) | mc_kl (per class, 64 partials each) | K_uu, factorization, inverse, K_ub, A | T (batched)
//   mc_cols (A read ONCE for all classes: C means, C variances per datum) | mc_ell | mc_finalize        -- a value-only call ends here --
//   mc_scale | W (k = C Mp) | mc_abar | mc_gm | G_c (batched, split-k) | mc_gls | Kubbar .. P, contractions: as sgp_svgp_elbo_batch
// Passes per step with gradients: A is read 6 times (T, cols, g_m, abar, G, S1) whatever C is; each of the C slices of T is read 4 times
// (cols, scale, W, G) and written twice (T, scale).
#include "sgp_dense.hpp"
#include "sgp_lik.hpp"
#include "sgp_svgp_shared.hpp"

namespace sgp {

static_assert(SGP_MAX_CLASSES == 16, "the class dispatch of mc_cols stops at 16");
constexpr int MC_ELL_BLOCKS = 256;  // x 64 threads: the likelihood's grid (stride 16384 data)

// LScat[r][c Mp + j] = tril(LS_c)[r][j] padded to Mp x Mp with a unit diagonal ; mp[c] = m_c zero padded ; status word <- 0
__global__ __launch_bounds__(256) void svgp_mc_prep_kernel(const double* __restrict__ LS, const double* __restrict__ m, int M, int Mp, int C,
                                                           double* __restrict__ LScat, double* __restrict__ mp, int* __restrict__ info) {
  const int cls = blockIdx.y;
  const int64_t total = (int64_t)Mp * Mp;
  LS += (int64_t)cls * M * M;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int r = (int)(e / Mp), c = (int)(e - (int64_t)r * Mp);
    double v = 0.0;
    if (r < M && c <= r) v = LS[(int64_t)r * M + c];
    else if (r >= M && r == c) v = 1.0;
    LScat[(int64_t)r * C * Mp + (int64_t)cls * Mp + c] = v;
    if (e < Mp) mp[(int64_t)cls * Mp + e] = e < M ? m[(int64_t)cls * M + e] : 0.0;
    if (e == 0 && cls == 0) info[0] = 0;
  }
}

// klpart[c][block] = partial of  sum m_c^2 - 2 sum log diag(LS_c) + ||tril(LS_c)||_F^2   (svgp_kl_kernel's arithmetic, class blockIdx.y)
__global__ __launch_bounds__(256) void svgp_mc_kl_kernel(const double* __restrict__ m, const double* __restrict__ LS, int M,
                                                         double* __restrict__ klpart) {
  __shared__ double red[4];
  m += (int64_t)blockIdx.y * M;
  LS += (int64_t)blockIdx.y * M * M;
  double s = 0.0;
  const int t = blockIdx.x * 256 + threadIdx.x, nt = gridDim.x * 256;
  for (int i = t; i < M; i += nt) s += m[i] * m[i] - 2.0 * log(LS[(int64_t)i * M + i]);
  for (int64_t e = t; e < (int64_t)M * M; e += nt) {
    const int r = (int)(e / M), c = (int)(e - (int64_t)r * M);
    if (c <= r) s = fma(LS[e], LS[e], s);
  }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) klpart[(int64_t)blockIdx.y * 64 + blockIdx.x] = s;
}

// One pass over A for ALL classes (block = 64 columns x 4 row groups, as svgp_cols_kernel): per column |A_b|^2 and, per class,
// mu[c][b] = sum_m A[m][b] mp[c][m], |T_c,b|^2; v[c][b] = sf2 - |A_b|^2 + |T_c,b|^2 as formed (1 in the padding).  CT >= C accumulators
// live in registers; the four row groups' partials are closed through LDS class by class in a fixed order.
template <int CT>
__global__ __launch_bounds__(256) void svgp_mc_cols_kernel(const double* __restrict__ A, const double* __restrict__ T,
                                                           const double* __restrict__ mp, int Mp, int Bp, int B, int C, double sf2,
                                                           double* __restrict__ mu, double* __restrict__ v) {
  __shared__ double pm[4][64], pa[4][64], pt[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int64_t mb = (int64_t)Mp * Bp;
  double sa = 0.0, sm[CT], st[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) sm[c] = st[c] = 0.0;
  for (int m = w; m < Mp; m += 4) {
    const double a = A[(int64_t)m * Bp + col];
    sa = fma(a, a, sa);
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) {
        const double t = T[c * mb + (int64_t)m * Bp + col];
        sm[c] = fma(a, mp[c * Mp + m], sm[c]);
        st[c] = fma(t, t, st[c]);
      }
  }
  pa[w][l] = sa;
  __syncthreads();
  const double saa = (pa[0][l] + pa[1][l]) + (pa[2][l] + pa[3][l]);
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C) {
      __syncthreads();  // the previous class's readers are done
      pm[w][l] = sm[c];
      pt[w][l] = st[c];
      __syncthreads();
      if (w == 0) {
        mu[(int64_t)c * Bp + col] = (pm[0][l] + pm[1][l]) + (pm[2][l] + pm[3][l]);
        v[(int64_t)c * Bp + col] = col < B ? sf2 - saa + ((pt[0][l] + pt[1][l]) + (pt[2][l] + pt[3][l])) : 1.0;
      }
    }
}

// The likelihood, one thread per datum.  The C means / variances / derivatives of a datum are NOT staged through LDS slots (as
// mc_rows_kernel's are): they already lie class-major in global memory, so the 64 data of a wave read and write consecutive doubles
// for every class, each value is read twice and written once against 20 x (C - 1) x 2 erfcx-class evaluations, and without LDS the
// kernel's occupancy is bounded by its registers alone.  One wave per workgroup spreads a minibatch of 4096 over 64 CUs.
// dvsum[b] = sum_c dv[c][b] in class order (the direct d/dsf2 and Abar's A term); part[block] = the block's sum of ell.
__global__ __launch_bounds__(64) void svgp_mc_ell_kernel(const double* __restrict__ y, const double* mu, const double* var, int B, int Bp,
                                                         int C, double var_floor, double eps, GHTable gh, double* dmu, double* dv,
                                                         double* __restrict__ dvsum, double* __restrict__ part) {
  double se = 0.0;
  for (int b = blockIdx.x * 64 + threadIdx.x; b < B; b += gridDim.x * 64) {
    double ell;
    lik_robustmax_pv(C, y[b], mu + b, var + b, Bp, var_floor, eps, gh, ell, dmu + b, dv + b);
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += dv[(int64_t)c * Bp + b];
    dvsum[b] = s;
    se += ell;
  }
  se = wave_sum(se);
  if (threadIdx.x == 0) part[blockIdx.x] = se;
}

// out = [F | sum ell | KL | status word as a double]; one thread, blocks then classes in index order
__global__ void svgp_mc_finalize_kernel(const double* __restrict__ part, const double* __restrict__ kl, int M, int B, int C, double N_total,
                                        const int* __restrict__ info, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double se = 0.0;
  for (int i = 0; i < MC_ELL_BLOCKS; ++i) se += part[i];
  double klv = 0.0;
  for (int c = 0; c < C; ++c) {
    double s = 0.0;
    for (int i = 0; i < 64; ++i) s += kl[c * 64 + i];
    klv += 0.5 * (s - (double)M);
  }
  out[0] = se / (double)B - klv / N_total;
  out[1] = se;
  out[2] = klv;
  out[3] = (double)info[0];
}

// in place: T_c <- T_c diag(vbar_c), vbar_c = dv_c / B (zero in the padded columns)
__global__ __launch_bounds__(256) void svgp_mc_scale_kernel(double* __restrict__ T, const double* __restrict__ dv, int Mp, int Bp, int B,
                                                            double invB) {
  const int64_t total = (int64_t)Mp * Bp;
  T += (int64_t)blockIdx.y * total;
  dv += (int64_t)blockIdx.y * Bp;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int b = (int)(e % Bp);
    T[e] = b < B ? T[e] * (dv[b] * invB) : 0.0;
  }
}

// Abar = sum_c mp_c mubar_c^T (class order) + 2 (W - A diag(sum_c vbar_c)),  W = sum_c Ls_c T_c diag(vbar_c)
__global__ __launch_bounds__(256) void svgp_mc_abar_kernel(const double* __restrict__ A, const double* __restrict__ W,
                                                           const double* __restrict__ mp, const double* __restrict__ dmu,
                                                           const double* __restrict__ dvsum, int Mp, int Bp, int B, int C, double invB,
                                                           double* __restrict__ Abar) {
  const int64_t total = (int64_t)Mp * Bp;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int m = (int)(e / Bp), b = (int)(e - (int64_t)m * Bp);
    double ab = 0.0;
    if (b < B) {
      for (int c = 0; c < C; ++c) ab = fma(mp[c * Mp + m], dmu[(int64_t)c * Bp + b] * invB, ab);
      ab += 2.0 * (W[e] - A[e] * (dvsum[b] * invB));
    }
    Abar[e] = ab;
  }
}

// g_m[c][m] = sum_b A[m][b] dmu[c][b] / B - m[c][m] / N      (one wave per row, class blockIdx.y; A shared)
__global__ __launch_bounds__(256) void svgp_mc_gm_kernel(const double* __restrict__ A, const double* __restrict__ dmu,
                                                         const double* __restrict__ m, int M, int Bp, int B, double invB, double invN,
                                                         double* __restrict__ g_m) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  dmu += (int64_t)blockIdx.y * Bp;
  double s = 0.0;
  for (int b = lane; b < B; b += 64) s = fma(A[(int64_t)row * Bp + b], dmu[b], s);
  s = wave_sum(s);
  if (lane == 0) g_m[(int64_t)blockIdx.y * M + row] = s * invB - m[(int64_t)blockIdx.y * M + row] * invN;
}

// g_LS[c] = tril(2 G_c) - (LS_c - diag(1 / diag LS_c)) / N   (M x M, ld M; strictly-upper part zero)
__global__ __launch_bounds__(256) void svgp_mc_gls_kernel(const double* __restrict__ G, int Mp, const double* __restrict__ LS, int M,
                                                          double invN, double* __restrict__ g_LS) {
  const int64_t total = (int64_t)M * M;
  G += (int64_t)blockIdx.y * Mp * Mp;
  LS += (int64_t)blockIdx.y * total;
  g_LS += (int64_t)blockIdx.y * total;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int r = (int)(e / M), c = (int)(e - (int64_t)r * M);
    double v = 0.0;
    if (c <= r) {
      v = 2.0 * G[(int64_t)r * Mp + c] - LS[e] * invN;
      if (c == r) v += invN / LS[e];
    }
    g_LS[e] = v;
  }
}

// probs[t][c] = (1 - eps) P(c largest) + eps / (C - 1) (1 - P(c largest)): one quadrature per (row, class), thread t C + c
__global__ __launch_bounds__(256) void svgp_mc_probs_kernel(const double* __restrict__ mu, const double* __restrict__ var, int64_t T, int Tp,
                                                            int C, double var_floor, double eps, GHTable gh, double* __restrict__ probs) {
  const int64_t total = T * C;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t t = e / C;
    const int c = (int)(e - t * C);
    double P[GH_N];
    const double p = robustmax_pv_nodes(C, c, mu + t, var + t, Tp, var_floor, gh, P);
    probs[e] = (1.0 - eps) * p + eps / (double)(C - 1) * (1.0 - p);
  }
}

struct SvgpMcWs {
  double *LScat, *mp, *kl, *Kp, *Linv, *tmp, *S1, *Q, *P, *G, *Kub, *A, *W, *Abar, *T, *mu, *v, *dmu, *dv, *dvsum, *part, *splitk, *kpart, *gzraw;
  int* flags;
  size_t bytes;
};
static SvgpMcWs carve_svgp_mc(void* ws, int Mp, int Bp, int M, int d, int C) {
  Carver c(ws);
  SvgpMcWs w;
  const size_t mm = (size_t)Mp * Mp, mb = (size_t)Mp * Bp;
  w.LScat = c.take<double>(C * mm);
  w.mp = c.take<double>((size_t)C * Mp);
  w.kl = c.take<double>((size_t)C * 64);
  w.Kp = c.take<double>(mm);
  w.Linv = c.take<double>(mm);
  w.tmp = c.take<double>(mm);
  w.S1 = c.take<double>(mm);
  w.Q = c.take<double>(mm);
  w.P = c.take<double>(mm);
  w.G = c.take<double>(C * mm);
  w.Kub = c.take<double>(mb);
  w.A = c.take<double>(mb);
  w.W = c.take<double>(mb);
  w.Abar = c.take<double>(mb);
  w.T = c.take<double>(C * mb);
  w.mu = c.take<double>((size_t)C * Bp);
  w.v = c.take<double>((size_t)C * Bp);
  w.dmu = c.take<double>((size_t)C * Bp);
  w.dv = c.take<double>((size_t)C * Bp);
  w.dvsum = c.take<double>(Bp);
  w.part = c.take<double>(MC_ELL_BLOCKS);
  w.splitk = c.take<double>((size_t)C * SVGP_SPLITK * mm);
  w.kpart = c.take<double>((size_t)2 * M * (d + 1));
  w.gzraw = c.take<double>((size_t)2 * M * d);
  w.flags = c.take<int>(potrf_scratch_ints(Mp));
  w.bytes = c.used();
  return w;
}

static bool mc_shape_ok(int64_t B, int M, int d, int C) {
  return B > 0 && B <= (1 << 20) && M > 0 && d > 0 && d <= SGP_MAX_DIM && M <= SGP_MAX_INDUCING && C >= 2 && C <= SGP_MAX_CLASSES;
}

// predict: the forward half on the rows Xb without labels; out = mean (C x B), g_m = var (C x B, as formed), g_LS = probs (B x C) or NULL
static int svgp_mc_impl(bool predict, const double* Xb, int64_t ldx, const double* yb, int64_t B, const double* Z, int64_t ldz,
                        const double* inv_ls, double sf2, double jitter, const double* m, const double* LS, int C, double eps,
                        int64_t N_total, int M, int d, int kernel_id, int with_grads, double* out, double* g_m, double* g_LS,
                        double* g_Z, double* g_ls, double* g_sf2, int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!Xb || (!yb && !predict) || !Z || !inv_ls || !m || !LS || !out || !info || B <= 0 || M <= 0 || d <= 0 || ldx < d || ldz < d ||
      N_total <= 0)
    return SGP_ERR_ARG;
  if (predict && !g_m) return SGP_ERR_ARG;
  if (C < 2 || C > SGP_MAX_CLASSES || !(eps > 0.0 && eps < 1.0) || !(sf2 > 0.0)) return SGP_ERR_ARG;
  if (kernel_id < 0 || kernel_id > SGP_KERNEL_MATERN52) return SGP_ERR_ARG;
  if (with_grads && (!g_m || !g_LS || !g_Z || !g_ls || !g_sf2)) return SGP_ERR_ARG;
  if (d > SGP_MAX_DIM || M > SGP_MAX_INDUCING || B > (1 << 20)) return SGP_ERR_DIM;
  const int Mp = padded_m(M), Bp = (int)round_up64(B, 64);
  SvgpMcWs w = carve_svgp_mc(ws, Mp, Bp, M, d, C);
  if (!ws || ws_bytes < w.bytes) return SGP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  static const GHTable gh = make_gh();
  SvgpThetaS th{};
  th.ka[0] = make_kern_args(inv_ls, sf2, d);
  th.s2[0] = 1.0;
  const double invB = 1.0 / (double)B, invN = 1.0 / (double)N_total, var_floor = sf2 * 0x1p-40;
  const int64_t mm = (int64_t)Mp * Mp, mb = (int64_t)Mp * Bp;
  const int gmm = grid_for_s(mm), gmb = grid_for_s(mb);

  // ---- forward ----------------------------------------------------------------------------------------------------
  svgp_mc_prep_kernel<<<dim3(gmm, C), 256, 0, st>>>(LS, m, M, Mp, C, w.LScat, w.mp, info);
  if (!predict) svgp_mc_kl_kernel<<<dim3(64, C), 256, 0, st>>>(m, LS, M, w.kl);
  switch (kernel_id) {
    case SGP_KERNEL_RBF: svgp_kuu_batch_kernel<SGP_KERNEL_RBF><<<dim3(gmm, 1), 256, 0, st>>>(Z, ldz, 0, th, jitter, M, Mp, w.Kp); break;
    case SGP_KERNEL_MATERN32: svgp_kuu_batch_kernel<SGP_KERNEL_MATERN32><<<dim3(gmm, 1), 256, 0, st>>>(Z, ldz, 0, th, jitter, M, Mp, w.Kp); break;
    default: svgp_kuu_batch_kernel<SGP_KERNEL_MATERN52><<<dim3(gmm, 1), 256, 0, st>>>(Z, ldz, 0, th, jitter, M, Mp, w.Kp); break;
  }
  potrf_lower_batch(w.Kp, w.Linv, Mp, Mp, 1, mm, info, w.flags, st);
  tri_inverse(w.Kp, w.Linv, w.tmp, Mp, Mp, st, 1, mm);
  switch (kernel_id) {
    case SGP_KERNEL_RBF: svgp_kub_batch_kernel<SGP_KERNEL_RBF><<<dim3(gmb, 1), 256, 0, st>>>(Z, ldz, 0, Xb, ldx, th, M, Mp, (int)B, Bp, w.Kub); break;
    case SGP_KERNEL_MATERN32: svgp_kub_batch_kernel<SGP_KERNEL_MATERN32><<<dim3(gmb, 1), 256, 0, st>>>(Z, ldz, 0, Xb, ldx, th, M, Mp, (int)B, Bp, w.Kub); break;
    default: svgp_kub_batch_kernel<SGP_KERNEL_MATERN52><<<dim3(gmb, 1), 256, 0, st>>>(Z, ldz, 0, Xb, ldx, th, M, Mp, (int)B, Bp, w.Kub); break;
  }
  GemmDesc a;  // A = L^-1 Kub
  a.A = w.Linv; a.lda = Mp; a.B = w.Kub; a.ldb = Bp; a.C = w.A; a.ldc = Bp;
  a.m = Mp; a.n = Bp; a.k = Mp; a.khi_mask = 1;
  gemm(a, st);
  GemmDesc t;  // T_c = Ls_c^T A   (class c of LScat: column offset c Mp, ld C Mp; A shared)
  t.A = w.LScat; t.lda = (int64_t)C * Mp; t.ta = true; t.B = w.A; t.ldb = Bp; t.C = w.T; t.ldc = Bp;
  t.m = Mp; t.n = Bp; t.k = Mp; t.klo_mask = 1;
  t.batch2 = C; t.s2A = Mp; t.s2B = 0; t.s2C = mb;
  gemm(t, st);
  if (C <= 4) svgp_mc_cols_kernel<4><<<Bp / 64, 256, 0, st>>>(w.A, w.T, w.mp, Mp, Bp, (int)B, C, sf2, w.mu, w.v);
  else svgp_mc_cols_kernel<16><<<Bp / 64, 256, 0, st>>>(w.A, w.T, w.mp, Mp, Bp, (int)B, C, sf2, w.mu, w.v);
  if (predict) {
    crop_copy(w.mu, Bp, out, B, C, (int)B, st);
    crop_copy(w.v, Bp, g_m, B, C, (int)B, st);
    if (g_LS) svgp_mc_probs_kernel<<<grid_for_s(B * C), 256, 0, st>>>(w.mu, w.v, B, Bp, C, var_floor, eps, gh, g_LS);
    return check_launch();
  }
  svgp_mc_ell_kernel<<<MC_ELL_BLOCKS, 64, 0, st>>>(yb, w.mu, w.v, (int)B, Bp, C, var_floor, eps, gh, w.dmu, w.dv, w.dvsum, w.part);
  svgp_mc_finalize_kernel<<<1, 64, 0, st>>>(w.part, w.kl, M, (int)B, C, (double)N_total, info, out);
  if (!with_grads) return check_launch();

  // ---- reverse ----------------------------------------------------------------------------------------------------
  svgp_mc_gm_kernel<<<dim3((M + 3) / 4, C), 256, 0, st>>>(w.A, w.dmu, m, M, Bp, (int)B, invB, invN, g_m);
  svgp_mc_scale_kernel<<<dim3(gmb, C), 256, 0, st>>>(w.T, w.dv, Mp, Bp, (int)B, invB);
  GemmDesc u;  // W = [Ls_0 | .. | Ls_C-1] [T_0 diag vbar_0 ; .. ; T_C-1 diag vbar_C-1]: the class sum inside ONE product, k = C Mp
  u.A = w.LScat; u.lda = (int64_t)C * Mp; u.B = w.T; u.ldb = Bp; u.C = w.W; u.ldc = Bp;
  u.m = Mp; u.n = Bp; u.k = C * Mp;
  gemm(u, st);
  svgp_mc_abar_kernel<<<gmb, 256, 0, st>>>(w.A, w.W, w.mp, w.dmu, w.dvsum, Mp, Bp, (int)B, C, invB, w.Abar);
  GemmDesc gl;  // G_c = A (T_c diag vbar_c)^T -> g_LS_c
  gl.A = w.A; gl.lda = Bp; gl.B = w.T; gl.ldb = Bp; gl.tb = true; gl.C = w.G; gl.ldc = Mp;
  gl.m = Mp; gl.n = Mp; gl.k = Bp;
  gl.batch2 = C; gl.s2A = 0; gl.s2B = mb; gl.s2C = mm;
  gemm_splitk(gl, SVGP_SPLITK, w.splitk, st);
  svgp_mc_gls_kernel<<<dim3(grid_for_s((int64_t)M * M), C), 256, 0, st>>>(w.G, Mp, LS, M, invN, g_LS);
  // from Abar on: sgp_svgp_elbo_batch's chain at S = 1
  GemmDesc bb;  // Kubbar = L^-T Abar (into W)
  bb.A = w.Linv; bb.lda = Mp; bb.ta = true; bb.B = w.Abar; bb.ldb = Bp; bb.C = w.W; bb.ldc = Bp;
  bb.m = Mp; bb.n = Bp; bb.k = Mp; bb.klo_mask = 1;
  gemm(bb, st);
  GemmDesc s1;  // S1 = Kubbar A^T ; Lbar = -tril(S1)
  s1.A = w.W; s1.lda = Bp; s1.B = w.A; s1.ldb = Bp; s1.tb = true; s1.C = w.S1; s1.ldc = Mp;
  s1.m = Mp; s1.n = Mp; s1.k = Bp;
  gemm_splitk(s1, SVGP_SPLITK, w.splitk, st);
  svgp_tril_batch_kernel<<<dim3(gmm, 1), 256, 0, st>>>(w.S1, Mp, -1.0, 0);
  GemmDesc q;  // Q = L^T Lbar ; Phi(Q)
  q.A = w.Kp; q.lda = Mp; q.ta = true; q.B = w.S1; q.ldb = Mp; q.C = w.Q; q.ldc = Mp;
  q.m = Mp; q.n = Mp; q.k = Mp; q.klo_mask = 3;
  gemm(q, st);
  svgp_tril_batch_kernel<<<dim3(gmm, 1), 256, 0, st>>>(w.Q, Mp, 1.0, 1);
  GemmDesc p1;  // tmp = L^-T Phi(Q)
  p1.A = w.Linv; p1.lda = Mp; p1.ta = true; p1.B = w.Q; p1.ldb = Mp; p1.C = w.tmp; p1.ldc = Mp;
  p1.m = Mp; p1.n = Mp; p1.k = Mp; p1.klo_mask = 3;
  gemm(p1, st);
  GemmDesc p2;  // P = tmp L^-1 ; Kuubar = sym(P), read in place by the contraction kernel
  p2.A = w.tmp; p2.lda = Mp; p2.B = w.Linv; p2.ldb = Mp; p2.C = w.P; p2.ldc = Mp;
  p2.m = Mp; p2.n = Mp; p2.k = Mp; p2.klo_mask = 2;
  gemm(p2, st);
  switch (kernel_id) {
    case SGP_KERNEL_RBF: svgp_kbwd_batch_kernel<SGP_KERNEL_RBF><<<dim3(2 * M, 1), 256, 0, st>>>(Z, ldz, Xb, ldx, th, w.W, w.P, M, Mp, Bp, (int)B, w.kpart, w.gzraw); break;
    case SGP_KERNEL_MATERN32: svgp_kbwd_batch_kernel<SGP_KERNEL_MATERN32><<<dim3(2 * M, 1), 256, 0, st>>>(Z, ldz, Xb, ldx, th, w.W, w.P, M, Mp, Bp, (int)B, w.kpart, w.gzraw); break;
    default: svgp_kbwd_batch_kernel<SGP_KERNEL_MATERN52><<<dim3(2 * M, 1), 256, 0, st>>>(Z, ldz, Xb, ldx, th, w.W, w.P, M, Mp, Bp, (int)B, w.kpart, w.gzraw); break;
  }
  svgp_kbwd_reduce_batch_kernel<<<dim3(grid_for_s((int64_t)M * d, 256), 1), 256, 0, st>>>(w.kpart, w.gzraw, M, th, w.dvsum, (int)B, Bp, invB, g_ls, g_sf2, g_Z);
  return check_launch();
}

}  // namespace sgp

using namespace sgp;

extern "C" size_t sgp_svgp_mc_workspace_bytes(int64_t B, int M, int d, int C) {
  if (!mc_shape_ok(B, M, d, C)) return 0;
  return carve_svgp_mc(nullptr, padded_m(M), (int)round_up64(B, 64), M, d, C).bytes;
}

extern "C" int sgp_svgp_mc_elbo(const double* Xb, int64_t ldx, const double* yb, int64_t B, const double* Z, int64_t ldz,
                                const double* inv_ls, double sf2, double jitter, const double* m, const double* LS, int C, double eps,
                                int64_t N_total, int M, int d, int kernel_id, int with_grads, double* out, double* g_m, double* g_LS,
                                double* g_Z, double* g_ls, double* g_sf2, int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  return svgp_mc_impl(false, Xb, ldx, yb, B, Z, ldz, inv_ls, sf2, jitter, m, LS, C, eps, N_total, M, d, kernel_id, with_grads, out, g_m,
                      g_LS, g_Z, g_ls, g_sf2, info, ws, ws_bytes, stream);
}

extern "C" int sgp_svgp_mc_predict(const double* Xs, int64_t ldxs, int64_t T, const double* Z, int64_t ldz, const double* inv_ls, double sf2,
                                   double jitter, const double* m, const double* LS, int C, double eps, int M, int d, int kernel_id,
                                   double* mean, double* var, double* probs, int* info, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  return svgp_mc_impl(true, Xs, ldxs, nullptr, T, Z, ldz, inv_ls, sf2, jitter, m, LS, C, eps, 1, M, d, kernel_id, 0, mean, var, probs,
                      nullptr, nullptr, nullptr, info, ws, ws_bytes, stream);
}
