// SGPMC with the multi-class robust-max likelihood (include/sgp.h: sgp_sgpmc_mc_rows, sgp_sgpmc_mc_tail): C latent GPs that share one
// kernel and one Z, whitened inducing values V = [v_1 .. v_C] (C x M, class-major).  Assembly, T = K' R, the contraction and the fixed-order
// slab reduction are sgp_suffstats_fwd.hip's own (the row pass starts with stream_rows_start, as sgp_sgpmc_lik.hip's), the sandwich of
// the tail is linv_sandwich (sgp_dense.hpp), an empty shard's outputs are sgpmc_lik_empty_launch's; new here:
//   mc_pad_v_kernel                                    V zero-padded to C x Mp
//   mc_rows_kernel                                     reads T ONCE for all classes: the C means and the variance of every datum, V staged
//                                                      through LDS by column blocks; the likelihood; dmu (C x N), dv, [sum ell | 0 | sum dv]
//   -- a value-only call and a moments-only call (y == NULL) end here --
//   mc_gpart_kernel, mc_gred_kernel                    g_c = sf2 T^T dmu_c for all classes in one read of T
//   mc_scale_kernel(+), contraction, slab reduction    G+ =  sf2^2 S+^T S+,  S+ = diag(sqrt(max(dv, 0))) T   (into the dead K'_fu block)
//   mc_scale_kernel(-), contraction, slab reduction    G- = -sf2^2 S-^T S-,  S- = diag(sqrt(max(-dv, 0))) T;  mc_add_kernel: G = G- + G+
//   mc_fold_kernel                                     T_out <- diag(dv) T - DMU V^T / (2 sf2): pass 2's T_in (see sgp.h)
// dv has BOTH signs under this likelihood (a datum the model gets wrong wants more variance), hence the two contractions: each is the
// existing positive semi-definite one, and their difference loses nothing against the scale sum_n |dv_n| a_n a_n^T of G itself.
// T is read 6 times per evaluation with adjoints (rows, g, two scalings, fold, and pass 2 reads the folded T), once without.
#include "sgp_common.hpp"
#include "sgp_stream.hpp"
#include "sgp_dense.hpp"
#include "sgp_ctx.hpp"
#include "sgp_lik.hpp"
#include "sgp_sgpmc_lik.hpp"

namespace sgp {

constexpr int MC_ROWS = 128;       // data rows per workgroup of the row pass (ASM_ROWS is a multiple of it)
constexpr int MC_V_STAGE = 2048;   // doubles of V kept in LDS at a time (16 KB): CT x CB with CB a multiple of 128 columns
static_assert(ASM_ROWS % MC_ROWS == 0, "the padded row count must be a multiple of the row pass's block");
static_assert(SGP_MAX_CLASSES == 16, "the class dispatch below stops at 16");

// the compile-time class count a call runs with: the smallest of {2, 3, 4, 8, 16} that holds C (V's rows beyond C are zeros in LDS)
static inline int mc_ct(int C) { return C <= 2 ? 2 : C <= 3 ? 3 : C <= 4 ? 4 : C <= 8 ? 8 : 16; }
// columns of V per LDS stage
static inline int mc_cb(int CT, int Mp) {
  int cb = MC_V_STAGE / CT / 128 * 128;
  if (cb < 128) cb = 128;
  return cb < Mp ? cb : Mp;
}
// row stride of the per-datum arrays in LDS: odd (no bank conflict between the rows of a wave), room for CT means and |t|^2
__host__ __device__ constexpr int mc_sa(int CT) { return (CT + 1) | 1; }

__global__ __launch_bounds__(256) void mc_pad_v_kernel(const double* __restrict__ V, int C, int M, int Mp, double* __restrict__ Vp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * Mp) return;
  const int c = i / Mp, m = i - c * Mp;
  Vp[i] = m < M ? V[(size_t)c * M + m] : 0.0;
}

// One workgroup per MC_ROWS rows.  Phase 1, per stage of CB columns: V's block goes to LDS (CT x CB), wave w owns rows [32 w, 32 w + 32),
// four at a time; a lane reads 16 bytes of each row per step of 128 columns and feeds CT dot products per row from LDS; the CT + 1 sums of
// a row are closed by the wave butterfly and added to the row's LDS slots in stage order.  Phase 2: one thread per row runs the likelihood
// on its LDS slots.  The partials [ell | dv] are added up by last_block_sums (sgp_common.hpp), in index order.  y == nullptr: moments
// only (mu_out, var_out), no ticket, nothing else written.
// LDS (dynamic): V stage (CT x CB) | means and |t|^2 (MC_ROWS x SA) | dmu (MC_ROWS x SA) | block_sum256's 4 words | the "I am last" word
template <int CT>
__global__ __launch_bounds__(256) void mc_rows_kernel(const double* __restrict__ T, const double* __restrict__ y,
                                                      const double* __restrict__ Vp, int64_t N, int64_t Npad, int Mp, int C, int CB,
                                                      double sf2, double eps, GHTable gh, double* __restrict__ dmu,
                                                      double* __restrict__ dv, double* __restrict__ mu_out, double* __restrict__ var_out,
                                                      double* __restrict__ dmu_pad, double* __restrict__ dv_pad, double* part,
                                                      int* __restrict__ counter, double* __restrict__ out) {
  constexpr int SA = mc_sa(CT);
  extern __shared__ double lds[];
  double* vsh = lds;
  double* acc = lds + (size_t)CT * CB;
  double* gsh = acc + MC_ROWS * SA;
  double* red = gsh + MC_ROWS * SA;
  double* last = red + 4;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t rbase = (int64_t)blockIdx.x * MC_ROWS;
  for (int i = tid; i < MC_ROWS * SA; i += 256) acc[i] = 0.0;
  for (int c0 = 0; c0 < Mp; c0 += CB) {
    const int ncol = Mp - c0 < CB ? Mp - c0 : CB;
    __syncthreads();  // the previous stage's readers are done with vsh (and acc is cleared)
    for (int i = tid; i < CT * ncol; i += 256) {
      const int c = i / ncol, j = i - c * ncol;
      vsh[c * CB + j] = c < C ? Vp[(size_t)c * Mp + c0 + j] : 0.0;
    }
    __syncthreads();
    for (int rr = 0; rr < MC_ROWS / 4; rr += 4) {
      const int r = wv * (MC_ROWS / 4) + rr;
      const double* t0 = T + (size_t)(rbase + r) * Mp + c0;
      double m0[CT], m1[CT], m2[CT], m3[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) m0[c] = m1[c] = m2[c] = m3[c] = 0.0;
      double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
      for (int j = 2 * lane; j < ncol; j += 128) {
        const d2 a0 = *reinterpret_cast<const d2*>(t0 + j);
        const d2 a1 = *reinterpret_cast<const d2*>(t0 + (size_t)Mp + j);
        const d2 a2 = *reinterpret_cast<const d2*>(t0 + 2 * (size_t)Mp + j);
        const d2 a3 = *reinterpret_cast<const d2*>(t0 + 3 * (size_t)Mp + j);
        q0 = fma(a0.y, a0.y, fma(a0.x, a0.x, q0));
        q1 = fma(a1.y, a1.y, fma(a1.x, a1.x, q1));
        q2 = fma(a2.y, a2.y, fma(a2.x, a2.x, q2));
        q3 = fma(a3.y, a3.y, fma(a3.x, a3.x, q3));
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          const d2 vv = *reinterpret_cast<const d2*>(vsh + c * CB + j);
          m0[c] = fma(a0.y, vv.y, fma(a0.x, vv.x, m0[c]));
          m1[c] = fma(a1.y, vv.y, fma(a1.x, vv.x, m1[c]));
          m2[c] = fma(a2.y, vv.y, fma(a2.x, vv.x, m2[c]));
          m3[c] = fma(a3.y, vv.y, fma(a3.x, vv.x, m3[c]));
        }
      }
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        m0[c] = wave_sum(m0[c]); m1[c] = wave_sum(m1[c]); m2[c] = wave_sum(m2[c]); m3[c] = wave_sum(m3[c]);
      }
      q0 = wave_sum(q0); q1 = wave_sum(q1); q2 = wave_sum(q2); q3 = wave_sum(q3);
      if (lane == 0) {  // this wave alone owns the four rows' slots
        double* a = acc + r * SA;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          a[c] += m0[c]; a[SA + c] += m1[c]; a[2 * SA + c] += m2[c]; a[3 * SA + c] += m3[c];
        }
        a[CT] += q0; a[SA + CT] += q1; a[2 * SA + CT] += q2; a[3 * SA + CT] += q3;
      }
    }
  }
  __syncthreads();
  const int64_t n = rbase + tid;
  double ell = 0.0, gv = 0.0;
  if (tid < MC_ROWS) {
    double* mrow = acc + tid * SA;
    double* grow = gsh + tid * SA;
    for (int c = 0; c < C; ++c) grow[c] = 0.0;
    if (n < N) {
      for (int c = 0; c < C; ++c) mrow[c] *= sf2;
      const double var = sf2 - (sf2 * sf2) * mrow[CT];
      if (mu_out)
        for (int c = 0; c < C; ++c) mu_out[(size_t)c * N + n] = mrow[c];
      if (var_out) var_out[n] = var;
      if (y) {
        const double floor_v = sf2 * 0x1p-40;
        const bool floored = var < floor_v;
        lik_robustmax(C, y[n], mrow, floored ? floor_v : var, eps, gh, ell, grow, gv);
        if (floored) gv = 0.0;
        for (int c = 0; c < C; ++c) dmu[(size_t)c * N + n] = grow[c];
        dv[n] = gv;
      }
    }
    if (y) {
      for (int c = 0; c < C; ++c) dmu_pad[(size_t)c * Npad + n] = grow[c];
      dv_pad[n] = gv;
    }
  }
  if (!y) return;
  double s[2];
  s[0] = block_sum256(ell, red);
  s[1] = block_sum256(gv, red);
  if (!last_block_sums(s, part, counter, red, last)) return;
  if (tid == 0) {
    out[0] = s[0];
    out[1] = 0.0;
    out[2] = s[1];
  }
}

// gpart[(block b, class c)][m] = sum over the block's ASM_ROWS rows of T[n][m] dmu_c[n], all classes from one read of T;
// grid = (Npad / ASM_ROWS, ceil(Mp / 256)), a thread per column, dmu of the block in LDS (read as wave-wide broadcasts)
template <int CT>
__global__ __launch_bounds__(256) void mc_gpart_kernel(const double* __restrict__ T, const double* __restrict__ dmu_pad, int64_t Npad,
                                                       int Mp, int C, double* __restrict__ gpart) {
  __shared__ double dsh[CT][ASM_ROWS];
  const int64_t rbase = (int64_t)blockIdx.x * ASM_ROWS;
#pragma unroll
  for (int c = 0; c < CT; ++c) dsh[c][threadIdx.x] = c < C ? dmu_pad[(size_t)c * Npad + rbase + threadIdx.x] : 0.0;
  __syncthreads();
  const int m = blockIdx.y * 256 + threadIdx.x;
  if (m >= Mp) return;
  const double* src = T + (size_t)rbase * Mp + m;
  double a[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) a[c] = 0.0;
  for (int i = 0; i < ASM_ROWS; ++i) {
    const double t = src[(size_t)i * Mp];
#pragma unroll
    for (int c = 0; c < CT; ++c) a[c] = fma(t, dsh[c][i], a[c]);
  }
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C) gpart[((size_t)blockIdx.x * C + c) * Mp + m] = a[c];
}
// g[c][m] = sf2 * the row blocks' partials added in block order
__global__ __launch_bounds__(256) void mc_gred_kernel(const double* __restrict__ gpart, int nblocks, int C, int M, int Mp, double sf2,
                                                      double* __restrict__ g) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * M) return;
  const int c = i / M, m = i - c * M;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += gpart[((size_t)b * C + c) * Mp + m];
  g[i] = sf2 * s;
}

// S_n <- sqrt(max(sign dv_n, 0)) T_n, zeros in the padding whatever dv holds; a NaN dv makes its row NaN in both signs.
constexpr int MC_SCALE_ROWS = 16;
constexpr int MC_SCALE_MAX_GROUPS = 4096;
__global__ __launch_bounds__(256) void mc_scale_kernel(const double* __restrict__ T, const double* __restrict__ dv_pad, int64_t N,
                                                       int64_t Npad, int M, int Mp, double sign, double* __restrict__ S) {
  __shared__ double s[MC_SCALE_ROWS];
  const int half = Mp >> 1, per = MC_SCALE_ROWS * half;
  for (int64_t g = blockIdx.x; g < Npad / MC_SCALE_ROWS; g += gridDim.x) {
    const int64_t r0 = g * MC_SCALE_ROWS;
    __syncthreads();
    if (threadIdx.x < MC_SCALE_ROWS) {
      const double x = sign * dv_pad[r0 + threadIdx.x];
      s[threadIdx.x] = x > 0.0 ? sqrt(x) : (x == x ? 0.0 : x);
    }
    __syncthreads();
    const d2* src = reinterpret_cast<const d2*>(T + (size_t)r0 * Mp);
    d2* dst = reinterpret_cast<d2*>(S + (size_t)r0 * Mp);
    for (int li = threadIdx.x; li < per; li += 256) {
      const int r = li / half, c = 2 * (li - r * half);
      const bool row_live = r0 + r < N;
      const d2 t = src[li];
      d2 o;
      o.x = (row_live && c < M) ? s[r] * t.x : 0.0;
      o.y = (row_live && c + 1 < M) ? s[r] * t.y : 0.0;
      dst[li] = o;
    }
  }
}

__global__ __launch_bounds__(256) void mc_add_kernel(double* __restrict__ G, const double* __restrict__ Gp, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) G[e] += Gp[e];
}

// T_n <- dv_n T_n - (1 / (2 sf2)) sum_c dmu_c[n] V_c in place, zeros in the padding.  grid = (row groups of 64, ceil(Mp / 512)): a thread
// keeps its two columns of V in registers and walks the rows; dmu and dv of a group come from LDS.
constexpr int MC_FOLD_ROWS = 64;
constexpr int MC_FOLD_MAX_GROUPS = 2048;
template <int CT>
__global__ __launch_bounds__(256) void mc_fold_kernel(double* __restrict__ T, const double* __restrict__ dmu_pad,
                                                      const double* __restrict__ dv_pad, const double* __restrict__ Vp, int64_t N,
                                                      int64_t Npad, int M, int Mp, int C, double h) {
  __shared__ double dsh[CT][MC_FOLD_ROWS];
  __shared__ double dvs[MC_FOLD_ROWS];
  const int col = (blockIdx.y * 256 + threadIdx.x) * 2;
  const bool col_ok = col < Mp;
  d2 v[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    v[c].x = 0.0; v[c].y = 0.0;
    if (col_ok && c < C) v[c] = *reinterpret_cast<const d2*>(Vp + (size_t)c * Mp + col);
  }
  for (int64_t g = blockIdx.x; g < Npad / MC_FOLD_ROWS; g += gridDim.x) {
    const int64_t r0 = g * MC_FOLD_ROWS;
    __syncthreads();
    for (int i = threadIdx.x; i < CT * MC_FOLD_ROWS; i += 256) {
      const int c = i / MC_FOLD_ROWS, r = i - c * MC_FOLD_ROWS;
      dsh[c][r] = c < C ? dmu_pad[(size_t)c * Npad + r0 + r] : 0.0;
    }
    if (threadIdx.x < MC_FOLD_ROWS) dvs[threadIdx.x] = dv_pad[r0 + threadIdx.x];
    __syncthreads();
    if (!col_ok) continue;
    for (int r = 0; r < MC_FOLD_ROWS; ++r) {
      d2* p = reinterpret_cast<d2*>(T + (size_t)(r0 + r) * Mp + col);
      const d2 t = *p;
      double sx = 0.0, sy = 0.0;
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        sx = fma(dsh[c][r], v[c].x, sx);
        sy = fma(dsh[c][r], v[c].y, sy);
      }
      const bool row_live = r0 + r < N;
      d2 o;
      o.x = (row_live && col < M) ? fma(dvs[r], t.x, -h * sx) : 0.0;
      o.y = (row_live && col + 1 < M) ? fma(dvs[r], t.y, -h * sy) : 0.0;
      *p = o;
    }
  }
}

template <typename F>
static inline void mc_dispatch(int CT, F&& f) {
  switch (CT) {
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    default: f(std::integral_constant<int, 16>()); break;
  }
}

struct McRowsWs {
  WhRowsWs wh;
  double *dmu_pad, *dv_pad, *part, *gpart, *Gpos, *Vp;
  int* counter;
  size_t bytes;
};
static McRowsWs carve_mc_rows(void* ws, const StreamPlan& p, int M, int C) {
  McRowsWs w;
  w.wh = carve_wh_rows(ws, p, true);
  Carver c(ws ? static_cast<char*>(ws) + w.wh.bytes : nullptr);
  const size_t rows = (size_t)(p.Npad > 0 ? p.Npad : 1);
  w.dmu_pad = c.take<double>((size_t)C * rows);
  w.dv_pad = c.take<double>(rows);
  w.part = c.take<double>(2 * (rows / MC_ROWS + 1));
  w.gpart = c.take<double>((rows / ASM_ROWS + 1) * (size_t)C * p.Mp);
  w.Gpos = c.take<double>((size_t)M * M);
  w.Vp = c.take<double>((size_t)C * p.Mp);
  w.counter = c.take<int>(1);
  w.bytes = w.wh.bytes + c.used();
  return w;
}

// ---- the tail ------------------------------------------------------------------------------------------------------------------
// Launch 1 (adjoints only), two jobs by block range as sgpmc_mid_kernel:
//  blocks [0, Mp / 16): one wave per row i of the padded layout writes, for c >= i, the two mirrored entries
//      S'[i][c] = S'[c][i] = sym(G)[i][c] - sum_k v_k[c] g_k[i] / 2      (0 in the padding; the class sum in class order)
//  the next C Mp / 64 blocks: w_k = L^-T v_k, a block per class and 64 columns, sixteen waves over the rows, partials added in wave order
__global__ __launch_bounds__(1024) void mc_mid_kernel(const double* __restrict__ G, const double* __restrict__ g,
                                                      const double* __restrict__ V, const double* __restrict__ Li, int C, int M, int Mp,
                                                      double* __restrict__ Sp, double* __restrict__ t) {
  __shared__ double part[16][64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nR = Mp / 16;
  if (b < nR) {
    const int i = b * 16 + wv;
    const bool live = i < M;
    for (int c = i + lane; c < Mp; c += 64) {
      double val = 0.0;
      if (live && c < M) {
        double s = 0.0;
        for (int k = 0; k < C; ++k) s = fma(V[(size_t)k * M + c], g[(size_t)k * M + i], s);
        val = fma(-0.5, s, 0.5 * (G[(int64_t)i * M + c] + G[(int64_t)c * M + i]));
      }
      Sp[(int64_t)i * Mp + c] = val;
      Sp[(int64_t)c * Mp + i] = val;
    }
    return;
  }
  const int nC = Mp / 64;
  const int k = (b - nR) / nC, col = ((b - nR) - k * nC) * 64 + lane;
  const double* v = V + (size_t)k * M;
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
    double a = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) a += part[q][lane];
    t[(size_t)k * Mp + col] = a;
  }
}

// The closing launch: blocks [0, nA) (adjoints only) write Kuubar = sym(R) cropped to M x M, bbar = the w_k and vbar = g - V; the last
// block adds v.v up over all classes in one fixed order and writes out.
__global__ __launch_bounds__(256) void mc_out_kernel(const double* __restrict__ R, const double* __restrict__ t,
                                                     const double* __restrict__ g, const double* __restrict__ V,
                                                     const double* __restrict__ rows, int C, int M, int Mp, double Nd, int nA,
                                                     double* __restrict__ Kuubar, double* __restrict__ bbar, double* __restrict__ vbar,
                                                     double* __restrict__ out) {
  if ((int)blockIdx.x == nA) {
    __shared__ double red[4];
    double a = 0.0;
    for (int i = threadIdx.x; i < C * M; i += 256) a = fma(V[i], V[i], a);
    const double vv = block_sum256(a, red);
    if (threadIdx.x != 0) return;
    const double LOG2PI = 1.8378770664093453;
    const double prior = -0.5 * vv - 0.5 * ((double)M * (double)C) * LOG2PI;
    out[SGP_SGPMC_OUT_F] = rows[0] + prior;
    out[SGP_SGPMC_OUT_DATA] = rows[0];
    out[SGP_SGPMC_OUT_PRIOR] = prior;
    out[SGP_SGPMC_OUT_S2BAR] = rows[1];
    out[SGP_SGPMC_OUT_KAPPABAR] = Nd > 0.0 ? rows[2] / Nd : 0.0;
    return;
  }
  const int64_t total = (int64_t)M * M;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)nA * 256) {
    const int r = (int)(e / M), c = (int)(e - (int64_t)r * M);
    Kuubar[e] = 0.5 * (R[(int64_t)r * Mp + c] + R[(int64_t)c * Mp + r]);
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < C * M; i += nA * 256) {
    const int k = i / M, m = i - k * M;
    bbar[i] = t[(size_t)k * Mp + m];
    vbar[i] = g[i] - V[i];
  }
}

struct McTailWs {
  double *Sp, *T, *R, *t;
  size_t bytes;
};
static McTailWs carve_mc_tail(void* ws, int Mp, int C) {
  Carver c(ws);
  McTailWs w;
  const size_t mm = (size_t)Mp * Mp;
  w.Sp = c.take<double>(mm);
  w.T = c.take<double>(mm);
  w.R = c.take<double>(mm);
  w.t = c.take<double>((size_t)C * Mp);
  w.bytes = c.used();
  return w;
}

static inline bool mc_classes_ok(int C) { return C >= 2 && C <= SGP_MAX_CLASSES; }

}  // namespace sgp

using namespace sgp;

extern "C" size_t sgp_sgpmc_mc_rows_workspace_bytes(int64_t N, int M, int d, int C) {
  if (!stream_shape_ok(N, M, d) || !mc_classes_ok(C)) return 0;
  StreamPlan p;
  if (!rows_plan(N, M, d, p)) return 0;
  return carve_mc_rows(nullptr, p, M, C).bytes;
}

extern "C" int sgp_sgpmc_mc_rows(const double* X, int64_t ldx, const double* y, const double* Z, int64_t ldz, const double* inv_ls,
                                 double sf2, const double* V, int C, double eps, int64_t N, int M, int d, int kernel_id,
                                 const double* kuu_linv, int want_adjoints, double* out, double* G, double* g, double* dmu, double* dv,
                                 double* mu, double* var, double* T_out, void* ws, size_t ws_bytes, sgp_stream_t stream) {
  const Ctx& cx = cur_ctx();
  if (!mc_classes_ok(C) || !(eps > 0.0 && eps < 1.0)) return SGP_ERR_ARG;
  if (want_adjoints && (!G || !g || (N > 0 && !y))) return SGP_ERR_ARG;
  if (N > 0 && y && (!dmu || !dv || !out)) return SGP_ERR_ARG;
  if (N > 0 && !y && (!mu || !var)) return SGP_ERR_ARG;
  if (N == 0 && !out) return SGP_ERR_ARG;
  // (the shared check asks for the data rows of a non-empty shard: X stands in for an absent y, which it never reads)
  if (const int bad = check_stream_args({Z, inv_ls, kuu_linv, V, T_out}, X, ldx, y ? y : X, ldz, N, M, d, kernel_id, false)) return bad;
  StreamPlan p;
  if (!rows_plan(N, M, d, p)) return SGP_ERR_WORKSPACE;
  McRowsWs w = carve_mc_rows(ws, p, M, C);
  if (!ws || ws_bytes < w.bytes) return SGP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const FwdWs& f = w.wh.f;
  if (p.Npad == 0) {
    sgpmc_lik_empty_launch(out, st);
    if (want_adjoints) {
      fill_zero(G, (size_t)M * M, st);
      fill_zero(g, (size_t)C * M, st);
    }
    return check_launch();
  }
  const int CT = mc_ct(C), CB = mc_cb(CT, p.Mp);
  // the prologue copies "y" into the padded ys the assembly's K'^T y partials read: neither is used here, any N readable doubles do
  stream_rows_start(p, kernel_id, make_kern_args(inv_ls, sf2, d), X, ldx, y ? y : X, Z, ldz, N, M, kuu_linv, w.wh, T_out, st);
  zero_ints(w.counter, 1, st);
  mc_pad_v_kernel<<<(C * p.Mp + 255) / 256, 256, 0, st>>>(V, C, M, p.Mp, w.Vp);
  static const GHTable gh = make_gh();
  const unsigned rgrid = (unsigned)(p.Npad / MC_ROWS);
  mc_dispatch(CT, [&](auto ct) {
    constexpr int K = decltype(ct)::value;
    const size_t lds = ((size_t)K * CB + 2 * (size_t)MC_ROWS * mc_sa(K) + 8) * sizeof(double);
    mc_rows_kernel<K><<<rgrid, 256, lds, st>>>(T_out, y, w.Vp, N, p.Npad, p.Mp, C, CB, sf2, eps, gh, dmu, dv, mu, var, w.dmu_pad, w.dv_pad,
                                               w.part, w.counter, out);
  });
  if (!want_adjoints || !y) return check_launch();
  const int nblocks = (int)(p.Npad / ASM_ROWS);
  mc_dispatch(CT, [&](auto ct) {
    constexpr int K = decltype(ct)::value;
    mc_gpart_kernel<K><<<dim3((unsigned)nblocks, (p.Mp + 255) / 256), 256, 0, st>>>(T_out, w.dmu_pad, p.Npad, p.Mp, C, w.gpart);
  });
  mc_gred_kernel<<<(C * M + 255) / 256, 256, 0, st>>>(w.gpart, nblocks, C, M, p.Mp, sf2, g);
  const int64_t sgroups = p.Npad / MC_SCALE_ROWS;
  const int sgrid = (int)(sgroups < MC_SCALE_MAX_GROUPS ? sgroups : MC_SCALE_MAX_GROUPS);
  const SplitMap smap = split_map(p.taper, p.Npad / NB, p.nsplit);
  // G = sum_n dv_n a_n a_n^T as the difference of two positive semi-definite contractions, the scaled rows in the dead K'_fu block
  mc_scale_kernel<<<sgrid, 256, 0, st>>>(T_out, w.dv_pad, N, p.Npad, M, p.Mp, 1.0, f.Kfu);
  launch_syrk(cx, f.Kfu, p.Mp, p.Npad / NB, smap, p.ntiles, p.nsplit, 0, f.slab, st);
  reduce_slabs(p, f.slab, p.nsplit, M, sf2 * sf2, w.Gpos, st);
  mc_scale_kernel<<<sgrid, 256, 0, st>>>(T_out, w.dv_pad, N, p.Npad, M, p.Mp, -1.0, f.Kfu);
  launch_syrk(cx, f.Kfu, p.Mp, p.Npad / NB, smap, p.ntiles, p.nsplit, 0, f.slab, st);
  reduce_slabs(p, f.slab, p.nsplit, M, -(sf2 * sf2), G, st);
  {
    const int64_t total = (int64_t)M * M, blocks = (total + 255) / 256;
    mc_add_kernel<<<(int)(blocks < 2048 ? blocks : 2048), 256, 0, st>>>(G, w.Gpos, total);
  }
  const int64_t fgroups = p.Npad / MC_FOLD_ROWS;
  const dim3 fgrid((unsigned)(fgroups < MC_FOLD_MAX_GROUPS ? fgroups : MC_FOLD_MAX_GROUPS), (p.Mp + 511) / 512);
  mc_dispatch(CT, [&](auto ct) {
    constexpr int K = decltype(ct)::value;
    mc_fold_kernel<K><<<fgrid, 256, 0, st>>>(T_out, w.dmu_pad, w.dv_pad, w.Vp, N, p.Npad, M, p.Mp, C, 0.5 / sf2);
  });
  return check_launch();
}

extern "C" size_t sgp_sgpmc_mc_workspace_bytes(int M, int C) {
  if (M <= 0 || M > SGP_MAX_INDUCING || !mc_classes_ok(C)) return 0;
  return carve_mc_tail(nullptr, padded_m(M), C).bytes;
}

extern "C" int sgp_sgpmc_mc_tail(const double* rows_out, const double* G, const double* g, const double* V, int C, int64_t N, int M,
                                 int with_adjoints, double* out, double* vbar, double* bbar, double* Kuubar, const double* kuu_linv,
                                 void* ws, size_t ws_bytes, sgp_stream_t stream) {
  if (!rows_out || !V || !out || M <= 0 || N < 0 || !mc_classes_ok(C)) return SGP_ERR_ARG;
  if (with_adjoints && (!G || !g || !vbar || !bbar || !Kuubar || !kuu_linv)) return SGP_ERR_ARG;
  if (M > SGP_MAX_INDUCING) return SGP_ERR_DIM;
  const int Mp = padded_m(M);
  McTailWs w = carve_mc_tail(ws, Mp, C);
  if (!ws || ws_bytes < w.bytes) return SGP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int nA = 0;
  if (with_adjoints) {
    mc_mid_kernel<<<Mp / 16 + C * (Mp / 64), 1024, 0, st>>>(G, g, V, kuu_linv, C, M, Mp, w.Sp, w.t);
    nA = linv_sandwich(w.Sp, kuu_linv, M, Mp, w.T, w.R, st);
  }
  mc_out_kernel<<<nA + 1, 256, 0, st>>>(w.R, w.t, g, V, rows_out, C, M, Mp, (double)N, nA, Kuubar, bbar, vbar, out);
  return check_launch();
}
