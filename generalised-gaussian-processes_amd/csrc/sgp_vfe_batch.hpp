// One collapsed (Titsias / VFE) sparse-GP bound with its complete gradient inside ONE 256-thread workgroup: the evaluation of
// sgp_vfe_eval_batch (sgp_vfe_batch.hip, include/sgp_vfe_batch.h: one problem per workgroup).  No inter-workgroup communication, no
// flags, no spins, no atomics.  The formulas are those at the head of tests/vfe_reference.py (the PyMC3 order of sgp_small_eval):
//
//   K = sf2 k'(Z, Z) + J I ; L = chol K ; A = L^-1 K_uf ; B = I + A A^T / s2 ; L_B = chol B ; u = A y ; c0 = L_B^-1 u ; g = B^-1 u
//   F = logmarg - trace                                                                       (a value-only call stops here)
//   Kbar_uf = L^-T [ W1 A + g y^T / s2^2 ] ,  W1 = (I - B^-1 - g g^T / s2^2) / s2
//   Kbar_uu = -1/2 L^-T C L^-1 ,              C  = B + B^-1 - 2 I + g g^T / s2^2
//   g_theta = sum Kbar_uf o dK_uf/dtheta + sum Kbar_uu o dK_uu/dtheta - N / (2 s2) dk(x, x)/dtheta ; g_s2 as the reference writes it.
//
// Everything stays in the WHITENED basis: a row tile's A_t = L^-1 K_uf,t is formed first, then the M x M adjoint factor W1 is applied,
// then L^-T.  No unwhitened M x M matrix is ever applied to K_uf (that order costs cond(K_uu), see the reference's docstring).
//
// LDS.  Mp = the size class of M (16, 32 or 64; identity in the padding), every M x M image Mp x (Mp + 2) doubles -- the bank-safe
// row stride of sgp_wg_dense.hpp.  P holds K -> L -> L^-1 for the whole call, Q holds B -> L_B -> L_B^-1 -> W1.  The two further
// images of the middle (B^-1 / C L^-1 and B / C / Kbar_uu) share their bytes with the two row tiles of the passes, which are never
// alive at the same time.  A row tile is TN = 2048 / Mp rows (128, 64, 32), stored TRANSPOSED, tile[n][m] with the images' stride: in
// every product  dst^T = Mimg src^T  the contraction index then runs along a row of both operands ("16 rows x 4 consecutive columns").
//   pass 1 : per tile K_uf,t -> A_t (matrix cores, clipped to L^-1's triangle) ; A A^T in register tiles ; u, sum A o A, y.y
//   middle : chol B, L_B^-1, c0, g, the value ; B^-1, W1, C, Kbar_uu and its contraction with dK_uu
//   pass 2 : per tile K_uf,t -> A_t -> W1 A_t + g y^T / s2^2 -> L^-T (.) = Kbar_uf,t ; contraction with dK_uf in the epilogue, by the
//            thread that assembled the entry (it kept k' and dk'/dr2 in registers)
// Thread <-> (inducing input m = tid / TPR, column class c = tid % TPR), TPR = 256 / Mp: in both passes a thread owns the 8 entries
// (m, c + TPR i) of a tile and, in the K_uu contraction, the column m of Kbar_uu -- so dF/dZ[m] is summed in registers, then over the
// TPR neighbouring lanes by a fixed butterfly.  Every sum has a fixed order that depends on (N, M, d) alone.
//
// The first part of this header is plain C++ (limits, size class, tile geometry, workspace, the theta-row check): a host program can
// include it without HIP (tests/native/vfe_batch_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/sgp.h"
#include "sgp_wg_dense.hpp"

#if defined(__HIPCC__)
#define SGP_VB_HD __host__ __device__
#else
#define SGP_VB_HD
#endif

namespace sgp {

constexpr int VB_MAXM = 64;             // Mp = 128 needs three 128 KB images at once
constexpr int64_t VB_MAXN = 65536;      // one workgroup walks all rows: the bound keeps a launch short
constexpr int VB_MAXD = 8;
constexpr int64_t VB_MAXP = (1 << 24) - 1;  // one workgroup per problem: P x 256 work-items stay below the 2^32 of one launch
constexpr int VB_XLD = VB_MAXD + 1;     // odd stride of the coordinate rows in LDS
constexpr int VB_TILE_ENTRIES = 2048;   // Mp x TN: 8 entries per thread
constexpr size_t VB_WS_UNIT = WG_WS_UNIT;  // the family's unit (sgp_wg_dense.hpp) under this header's name

// The size class of M (0: none): the launch picks the kernel instantiation by it
SGP_VB_HD constexpr int vb_size_class(int M) { return M < 1 || M > VB_MAXM ? 0 : (M <= 16 ? 16 : (M <= 32 ? 32 : 64)); }
// Rows per tile of a class, threads that share one inducing input, and tiles that cover N rows: the kernel's LDS layout, its thread map
// and its two row loops are written from these three
SGP_VB_HD constexpr int vb_tile_rows(int Mp) { return VB_TILE_ENTRIES / Mp; }
SGP_VB_HD constexpr int vb_threads_per_row(int Mp) { return 256 / Mp; }
SGP_VB_HD constexpr int vb_tiles(int N, int Mp) { return (N + vb_tile_rows(Mp) - 1) / vb_tile_rows(Mp); }

// SGP_OK, or what the entry points refuse a shape with: SGP_ERR_ARG before SGP_ERR_DIM
SGP_VB_HD inline int vb_check(int64_t P, int64_t N, int M, int d, int kernel_id) {
  if (P <= 0 || N <= 0 || M <= 0 || d <= 0) return SGP_ERR_ARG;
  if (kernel_id < 0 || kernel_id > SGP_KERNEL_MATERN52) return SGP_ERR_ARG;  // composite kernels: out of scope
  if (N > VB_MAXN || M > VB_MAXM || d > VB_MAXD || P > VB_MAXP) return SGP_ERR_DIM;
  return SGP_OK;
}

// The workspace.  It is a PLACEHOLDER: a problem lives in its workgroup's LDS and the kernel never reads or writes the buffer.  The one
// aligned unit keeps the convention of the library's other entry points (a query that answers 0 for an unsupported shape, a non-NULL
// buffer of at least that size) so that a later kernel of this family, M <= 128 with an image in global scratch, can grow it without a
// change of the ABI.
SGP_VB_HD inline size_t vb_workspace_bytes(int64_t P, int64_t N, int M, int d) {
  return vb_check(P, N, M, d, 0) == SGP_OK ? VB_WS_UNIT : 0;
}

// A theta row [ls_1..d | sf2 | s2] is usable when every entry is a positive finite number (NaN fails every comparison)
SGP_VB_HD inline bool vb_theta_ok(const double* th, int n) {
  bool ok = true;
  for (int q = 0; q < n; ++q) ok = ok && th[q] > 0.0 && th[q] <= 1.7976931348623157e308;
  return ok;
}

}  // namespace sgp

#if defined(__HIPCC__)
#include "sgp_common.hpp"

namespace sgp {

template <int MP>
struct VbShared {
  static constexpr int LD = MP + 2, TN = vb_tile_rows(MP);
  double P[MP][LD];  // K -> L -> L^-1
  double Q[MP][LD];  // B (lower) -> L_B -> L_B^-1 -> W1
  union {
    struct {
      double R[MP][LD];  // B^-1, then C L^-1
      double S[MP][LD];  // B, then C, then Kbar_uu
    } mid;
    struct {
      double KT[TN][LD];  // K_uf,t^T, then (W1 A_t + g y^T / s2^2)^T
      double AT[TN][LD];  // A_t^T, then Kbar_uf,t^T
    } tile;
  } u;
  double z[MP][VB_XLD];  // z_m / ls: the coordinates are scaled once, differences are formed from the scaled values
  double x[TN][VB_XLD];  // the tile's rows, scaled the same way
  double y[TN];
  double uv[MP], c0[MP], g[MP];
  double ils[VB_MAXD];  // 1 / ls_q (zero past d)
  double red[4];
  int bad;
};
static_assert(sizeof(VbShared<64>) <= 160 * 1024, "the large class must fit the CU's LDS");
static_assert(2 * sizeof(VbShared<32>) <= 160 * 1024, "two workgroups of the middle class per CU");
static_assert(2 * sizeof(VbShared<16>) <= 160 * 1024, "two workgroups of the small class per CU");
static_assert(VbShared<16>::TN >= 64, "the small class parks its four partial 16 x 16 tiles in the first 64 rows of a row tile");

enum { VB_FULL = 0, VB_LOWER = 1, VB_UPPER = 2 };

// Cholesky of the Mp x Mp image in place (lower; zeros above the diagonal of every diagonal block), right-looking by 16-column
// panels -- sgp_exact_batch.hpp's factorization without its right-hand side.  A pivot of a row below n_live that is not above `gate`
// (NaN included) is reported once in *bad as bad_base + its 1-based index; the factorization continues on a unit pivot.  Ends on a
// barrier.
template <int MP>
__device__ __forceinline__ void vb_chol(double (*Mt)[MP + 2], int n_live, double gate, int bad_base, int* bad) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  constexpr int nb = MP / 16;
  for (int pb = 0; pb < nb; ++pb) {
    const int c0 = 16 * pb;
    if (wave == 0) {  // the diagonal block: lane <-> row (the four lane groups hold copies), columns exchanged by shuffles
      double a[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) a[k] = Mt[c0 + l15][c0 + k];
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        double dj = __shfl(a[jj], jj, 64);
        if (c0 + jj < n_live && !(dj > gate)) {
          if (lane == 0 && *bad == 0) *bad = bad_base + c0 + jj + 1;
          dj = 1.0;
        }
        const double piv = sqrt(dj);
        const double l = (l15 == jj) ? piv : a[jj] / piv;
        a[jj] = l;
#pragma unroll
        for (int k = jj + 1; k < 16; ++k) a[k] = fma(-l, __shfl(l, k, 64), a[k]);
      }
      if (lane < 16) {
#pragma unroll
        for (int k = 0; k < 16; ++k) Mt[c0 + l15][c0 + k] = (k <= l15) ? a[k] : 0.0;
      }
    }
    __syncthreads();
    const int nbelow = MP - c0 - 16;
    if (tid < nbelow) {  // the rows below: thread <-> row, x = row D^-T by substitution
      const int i = c0 + 16 + tid;
      double x[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) x[k] = Mt[i][c0 + k];
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        double s = x[jj];
#pragma unroll
        for (int k = 0; k < jj; ++k) s = fma(-x[k], Mt[c0 + jj][c0 + k], s);
        x[jj] = s / Mt[c0 + jj][c0 + jj];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) Mt[i][c0 + k] = x[k];
    }
    __syncthreads();
    {  // rank-16 update of the trailing lower-triangle tiles on the matrix cores
      const int m = nb - pb - 1;
      for (int t = wave; t < m * (m + 1) / 2; t += 4) {
        int ri = 0;
        while ((ri + 1) * (ri + 2) / 2 <= t) ++ri;
        const int rj = t - ri * (ri + 1) / 2;
        const int i0 = 16 * (pb + 1 + ri), j0 = 16 * (pb + 1 + rj);
        d4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = Mt[i0 + l4 + 4 * r][j0 + l15];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma16(-Mt[i0 + l15][c0 + 4 * s + l4], Mt[j0 + l15][c0 + 4 * s + l4], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) Mt[i0 + l4 + 4 * r][j0 + l15] = acc[r];
      }
    }
    __syncthreads();
  }
}

// The inverse of the lower-triangular image in place, block column by block column from the right (sgp_exact_batch.hpp's eb_invert):
// Inv[below][J] = -Inv[below][below] L[below][J] Inv[J][J].  Ends on a barrier.
template <int MP>
__device__ __forceinline__ void vb_invert(double (*Mt)[MP + 2]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  constexpr int nb = MP / 16;
  for (int J = nb - 1; J >= 0; --J) {
    const int c0 = 16 * J, m = nb - 1 - J;  // m <= 3: one tile per wave
    d4 T = {0.0, 0.0, 0.0, 0.0};
    if (wave < m) {
      const int i0 = 16 * (J + 1 + wave);
      for (int k0 = c0 + 16; k0 <= i0; k0 += 16) {
#pragma unroll
        for (int s = 0; s < 4; ++s) T = mfma16(Mt[i0 + l15][k0 + 4 * s + l4], Mt[k0 + 4 * s + l4][c0 + l15], T);
      }
    }
    double xinv[16];  // wave 3, lane c < 16: column c of the inverse of the diagonal block (zero above the diagonal)
    if (wave == 3) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        double s = (r == l15) ? 1.0 : 0.0;
#pragma unroll
        for (int q = 0; q < r; ++q) s = fma(-Mt[c0 + r][c0 + q], xinv[q], s);
        xinv[r] = s / Mt[c0 + r][c0 + r];
      }
    }
    __syncthreads();
    if (wave < m) {
      const int i0 = 16 * (J + 1 + wave);
#pragma unroll
      for (int r = 0; r < 4; ++r) Mt[i0 + l4 + 4 * r][c0 + l15] = T[r];
    }
    if (wave == 3 && lane < 16) {
#pragma unroll
      for (int r = 0; r < 16; ++r) Mt[c0 + r][c0 + l15] = xinv[r];
    }
    __syncthreads();
    if (wave < m) {  // tile <- -T Inv[J][J]: a wave reads its own tile whole, then overwrites it
      const int i0 = 16 * (J + 1 + wave);
      double a[4], b[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        a[s] = -Mt[i0 + l15][c0 + 4 * s + l4];
        b[s] = Mt[c0 + 4 * s + l4][c0 + l15];
      }
      d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = mfma16(a[s], b[s], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) Mt[i0 + l4 + 4 * r][c0 + l15] = acc[r];
    }
    __syncthreads();
  }
}

// dst = alpha op(A) B over Mp x Mp images, op = transpose with TA; wave <-> output tiles wave, wave + 4, ...  No barrier inside.
template <int MP, bool TA>
__device__ __forceinline__ void vb_img_mm(double (*dst)[MP + 2], const double (*A)[MP + 2], const double (*B)[MP + 2], double alpha) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  constexpr int NI = MP / 16;
  for (int t = wave; t < NI * NI; t += 4) {
    const int i0 = 16 * (t / NI), j0 = 16 * (t % NI);
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < MP; k0 += 16) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = k0 + 4 * s + l4;
        acc = mfma16(TA ? A[k][i0 + l15] : A[i0 + l15][k], B[k][j0 + l15], acc);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[i0 + l4 + 4 * r][j0 + l15] = alpha * acc[r];
  }
}

// One row tile through an M x M factor, both tiles transposed:  dst[n][m] = sum_k op(Mimg)[m][k] src[n][k]  (+ gv[m] yv[n] rs with
// gv != nullptr).  TRI clips the contraction to the factor's triangle (VB_LOWER: k <= m's block, VB_UPPER: k >= m's block).  The 8
// output tiles go two to a wave so that the clipped costs balance.  No barrier inside; dst and src are different buffers.
template <int MP, int TRI, bool TA>
__device__ __forceinline__ void vb_tile_mm(double (*dst)[MP + 2], const double (*Mimg)[MP + 2], const double (*src)[MP + 2],
                                           const double* gv, const double* yv, double rs) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  constexpr int NI = MP / 16;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    int bi, bj;
    if constexpr (NI == 4) {
      bi = u ? 3 - wave : wave;
      bj = u;
    } else if constexpr (NI == 2) {
      bi = u;
      bj = wave;
    } else {
      bi = 0;
      bj = wave + 4 * u;
    }
    const int i0 = 16 * bi, j0 = 16 * bj;
    const int klo = TRI == VB_UPPER ? i0 : 0, khi = TRI == VB_LOWER ? i0 + 16 : MP;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = klo; k0 < khi; k0 += 16) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = k0 + 4 * s + l4;
        acc = mfma16(TA ? Mimg[k][i0 + l15] : Mimg[i0 + l15][k], src[j0 + l15][k], acc);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = i0 + l4 + 4 * r, n = j0 + l15;
      dst[n][m] = gv ? fma(gv[m] * rs, yv[n], acc[r]) : acc[r];
    }
  }
}

struct VbArgs {
  const double *X, *Y, *Z, *theta;
  int64_t x_stride, ldx, y_stride, z_stride, ldz;
  const int *ix, *iy, *iz;
  int N, M, d, want_grad;
  double jitter;
  double *out, *gz;
  int* info;
};

template <int MP>
__device__ __forceinline__ void vb_fail(const VbArgs& a, int64_t p, int bad) {
  const double nan = __builtin_nan("");
  const int tid = threadIdx.x;
  if (tid < a.d + 5) a.out[p * (a.d + 5) + tid] = nan;
  if (a.gz && a.want_grad) {
    for (int e = tid; e < a.M * a.d; e += 256) a.gz[p * (int64_t)(a.M * a.d) + e] = nan;
  }
  if (tid == 0) a.info[p] = bad;
}

// The row tile at t0 into LDS, scaled by 1 / ls (zero past N); the caller synchronises
template <int MP>
__device__ __forceinline__ void vb_load_rows(VbShared<MP>& sh, const double* __restrict__ Xp, int64_t ldx, const double* __restrict__ Yp,
                                             int t0, int N, int d) {
  constexpr int TN = VbShared<MP>::TN;
  const int tid = threadIdx.x;
  for (int e = tid; e < TN * d; e += 256) {
    const int n = e / d, q = e - n * d;
    sh.x[n][q] = t0 + n < N ? Xp[(int64_t)(t0 + n) * ldx + q] * sh.ils[q] : 0.0;
  }
  if (tid < TN) sh.y[tid] = t0 + tid < N ? Yp[t0 + tid] : 0.0;
}

template <int KID, int MP>
__device__ __forceinline__ void vb_eval(VbShared<MP>& sh, const VbArgs& a, int64_t p) {
  constexpr int TN = vb_tile_rows(MP), TPR = vb_threads_per_row(MP), NI = MP / 16, NE = 8;
  constexpr int NACC = NI == 4 ? 4 : 1;
  static_assert(TN * MP == 256 * NE && MP / TPR * TPR == MP, "8 entries per thread");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int N = a.N, M = a.M, d = a.d;
  const int n_tiles = vb_tiles(N, MP);
  const int mo = tid / TPR, co = tid % TPR;  // this thread's inducing input and column class
  const double* Xp = a.X + (int64_t)(a.ix ? a.ix[p] : 0) * a.x_stride;
  const double* Yp = a.Y + (int64_t)(a.iy ? a.iy[p] : 0) * a.y_stride;
  const double* Zp = a.Z + (int64_t)(a.iz ? a.iz[p] : 0) * a.z_stride;
  const double* th = a.theta + p * (d + 2);
  double* out = a.out + p * (d + 5);
  const double nan = __builtin_nan("");

  if (tid == 0) sh.bad = vb_theta_ok(th, d + 2) ? 0 : 1;
  if (tid < VB_MAXD) sh.ils[tid] = tid < d ? 1.0 / th[tid] : 0.0;
  for (int e = tid; e < MP * d; e += 256) {
    const int i = e / d, q = e - i * d;
    sh.z[i][q] = i < M ? Zp[(int64_t)i * a.ldz + q] * (1.0 / th[q]) : 0.0;
  }
  __syncthreads();
  if (sh.bad != 0) {  // (uniform over the workgroup)
    vb_fail<MP>(a, p, sh.bad);
    return;
  }
  const double sf2 = th[d], s2 = th[d + 1];

  // ---- K = sf2 k'(Z, Z) + J I: lower triangle, zero above it, identity in the padding ----
  for (int e = tid; e < MP * MP; e += 256) {
    const int i = e / MP, j = e - i * MP;
    double v = 0.0;
    if (i < M && j <= i) {
      double r2 = 0.0;
#pragma unroll
      for (int q = 0; q < VB_MAXD; ++q) {
        if (q < d) {
          const double df = sh.z[i][q] - sh.z[j][q];
          r2 = fma(df, df, r2);
        }
      }
      double kp, hp;
      kprofile_grad<KID>(r2, kp, hp);
      v = sf2 * kp;
      if (i == j) v += a.jitter;
    } else if (i == j) {
      v = 1.0;
    }
    sh.P[i][j] = v;
  }
  __syncthreads();
  // A pivot at or below 8 M 2^-53 times the diagonal of K is rounding noise of the updates that formed it
  vb_chol<MP>(sh.P, M, (sf2 + a.jitter) * (8.0 * (double)M) * 0x1p-53, 0, &sh.bad);
  if (sh.bad != 0) {
    vb_fail<MP>(a, p, sh.bad);
    return;
  }
  vb_invert<MP>(sh.P);

  // ---- pass 1: A_t = L^-1 K_uf,t ; A A^T ; u = A y ; sum A o A ; y.y ----
  d4 acc[NACC];
#pragma unroll
  for (int q = 0; q < NACC; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
  double pu = 0.0, pa2 = 0.0, pyy = 0.0;
  const int kperm = 8 * (l4 & 1) + 4 * (l4 >> 1);  // both operands of A A^T run down a column: sgp_wg_dense.hpp's row permutation
  for (int it = 0; it < n_tiles; ++it) {
    const int t0 = it * TN;
    vb_load_rows<MP>(sh, Xp, a.ldx, Yp, t0, N, d);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int n = co + TPR * i;
      double v = 0.0;
      if (mo < M && t0 + n < N) {
        double r2 = 0.0;
#pragma unroll
        for (int q = 0; q < VB_MAXD; ++q) {
          if (q < d) {
            const double df = sh.z[mo][q] - sh.x[n][q];
            r2 = fma(df, df, r2);
          }
        }
        double kp, hp;
        kprofile_grad<KID>(r2, kp, hp);
        v = sf2 * kp;
      }
      sh.u.tile.KT[n][mo] = v;
    }
    if (tid < TN) pyy = fma(sh.y[tid], sh.y[tid], pyy);
    __syncthreads();
    vb_tile_mm<MP, VB_LOWER, false>(sh.u.tile.AT, sh.P, sh.u.tile.KT, nullptr, nullptr, 0.0);
    __syncthreads();
    if constexpr (NI == 1) {  // one output tile: the four waves split the rows
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double* row = &sh.u.tile.AT[32 * wave + 16 * h + kperm + s][0];
          acc[0] = mfma16(row[l15], row[l15], acc[0]);
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < NACC; ++q) {
        const int t = wave + 4 * q, i0 = 16 * (t / NI), j0 = 16 * (t % NI);
        for (int n0 = 0; n0 < TN; n0 += 16) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const double* row = &sh.u.tile.AT[n0 + kperm + s][0];
            acc[q] = mfma16(row[i0 + l15], row[j0 + l15], acc[q]);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int n = co + TPR * i;
      const double v = sh.u.tile.AT[n][mo];
      pu = fma(v, sh.y[n], pu);
      pa2 = fma(v, v, pa2);
    }
    __syncthreads();
  }
#pragma unroll
  for (int o = TPR / 2; o > 0; o >>= 1) pu += __shfl_xor(pu, o, 64);
  if (co == 0) sh.uv[mo] = pu;
  const double sumA2 = block_sum256(pa2, sh.red);
  const double yy = block_sum256(pyy, sh.red);
  if constexpr (NI == 1) {  // the four waves' partial tiles, added in wave order
#pragma unroll
    for (int r = 0; r < 4; ++r) sh.u.tile.KT[16 * wave + l4 + 4 * r][l15] = acc[0][r];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = l4 + 4 * r;
        acc[0][r] = (sh.u.tile.KT[i][l15] + sh.u.tile.KT[16 + i][l15]) + (sh.u.tile.KT[32 + i][l15] + sh.u.tile.KT[48 + i][l15]);
      }
    }
  }
  __syncthreads();  // the tiles are dead: their bytes become the images R and S
  const double rs2 = 1.0 / s2;
#pragma unroll
  for (int q = 0; q < NACC; ++q) {
    const int t = wave + 4 * q;
    if (t < NI * NI) {
      const int i0 = 16 * (t / NI), j0 = 16 * (t % NI);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + l4 + 4 * r, j = j0 + l15;
        const double b = fma(acc[q][r], rs2, i == j ? 1.0 : 0.0);
        sh.u.mid.S[i][j] = b;
        sh.Q[i][j] = j <= i ? b : 0.0;
      }
    }
  }
  __syncthreads();

  // ---- the middle: L_B, L_B^-1, c0, g, the value ----
  // In exact arithmetic every pivot of B = I + A A^T / s2 is at least 1: one at or below 1/2 has been lost to rounding
  vb_chol<MP>(sh.Q, M, 0.5, M, &sh.bad);
  if (sh.bad != 0) {
    vb_fail<MP>(a, p, sh.bad);
    return;
  }
  const double logdet = block_sum256(tid < M ? log(sh.Q[tid][tid]) : 0.0, sh.red);
  vb_invert<MP>(sh.Q);
  if (tid < MP) {
    double s = 0.0;
    for (int k = 0; k <= tid; ++k) s = fma(sh.Q[tid][k], sh.uv[k], s);
    sh.c0[tid] = s;
  }
  __syncthreads();
  double cc = 0.0;
  if (tid < MP) {
    double s = 0.0;
    for (int k = tid; k < MP; ++k) s = fma(sh.Q[k][tid], sh.c0[k], s);
    sh.g[tid] = s;
    cc = sh.c0[tid] * sh.c0[tid];
  }
  cc = block_sum256(cc, sh.red);
  const double dN = (double)N;
  const double kappa = dN * sf2;
  const double logmarg = -(0.5 * dN * 1.8378770664093453 + 0.5 * dN * log(s2) + logdet + 0.5 * (yy / s2 - cc / (s2 * s2)));
  const double trace = (kappa - sumA2) / (2.0 * s2);
  const double F = logmarg - trace;
  if (!a.want_grad) {
    if (tid < d + 2) out[1 + tid] = nan;
    if (tid == 0) {
      out[0] = F;
      out[d + 3] = logmarg;
      out[d + 4] = trace;
      a.info[p] = 0;
    }
    return;
  }

  // ---- B^-1 = L_B^-T L_B^-1 ; W1 -> Q ; C -> S ; Kbar_uu = -1/2 L^-T C L^-1 -> S ----
  vb_img_mm<MP, true>(sh.u.mid.R, sh.Q, sh.Q, 1.0);
  __syncthreads();
  double trb = 0.0, ug = 0.0;
  if (tid < M) {
    trb = sh.u.mid.R[tid][tid];
    ug = sh.uv[tid] * sh.g[tid];
  }
  trb = block_sum256(trb, sh.red);
  ug = block_sum256(ug, sh.red);
  const double rs4 = rs2 * rs2;
  for (int e = tid; e < MP * MP; e += 256) {
    const int i = e / MP, j = e - i * MP;
    const double dl = i == j ? 1.0 : 0.0;
    const double binv = sh.u.mid.R[i][j], gg = sh.g[i] * sh.g[j] * rs4;
    sh.u.mid.S[i][j] = sh.u.mid.S[i][j] + binv - 2.0 * dl + gg;
    sh.Q[i][j] = (dl - binv - gg) * rs2;
  }
  __syncthreads();
  vb_img_mm<MP, false>(sh.u.mid.R, sh.u.mid.S, sh.P, 1.0);
  __syncthreads();
  vb_img_mm<MP, true>(sh.u.mid.S, sh.P, sh.u.mid.R, -0.5);
  __syncthreads();

  // ---- the contraction of Kbar_uu with dK_uu: this thread's column mo, rows co, co + TPR, ... (z_mo moves rows and columns) ----
  double gls[VB_MAXD], gzz[VB_MAXD], gsf = 0.0;
#pragma unroll
  for (int q = 0; q < VB_MAXD; ++q) gls[q] = gzz[q] = 0.0;
  if (mo < M) {
    for (int m = co; m < M; m += TPR) {
      const double kb = sh.u.mid.S[m][mo], kz = kb + sh.u.mid.S[mo][m];
      double r2 = 0.0;
#pragma unroll
      for (int q = 0; q < VB_MAXD; ++q) {
        if (q < d) {
          const double df = sh.z[mo][q] - sh.z[m][q];
          r2 = fma(df, df, r2);
        }
      }
      double kp, hp;
      kprofile_grad<KID>(r2, kp, hp);
      gsf = fma(kb, kp, gsf);
      const double h = sf2 * hp, e1 = kb * h, ez = kz * h;
#pragma unroll
      for (int q = 0; q < VB_MAXD; ++q) {
        if (q < d) {
          const double df = sh.z[mo][q] - sh.z[m][q];
          gls[q] = fma(e1 * df, df, gls[q]);
          gzz[q] = fma(ez, df, gzz[q]);
        }
      }
    }
  }
  __syncthreads();  // R and S are dead: their bytes become the tiles again

  // ---- pass 2: Kbar_uf,t = L^-T (W1 A_t + g y_t^T / s2^2), contracted with dK_uf ----
  double pag = 0.0;
  for (int it = 0; it < n_tiles; ++it) {
    const int t0 = it * TN;
    vb_load_rows<MP>(sh, Xp, a.ldx, Yp, t0, N, d);
    __syncthreads();
    double kpv[NE], hpv[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int n = co + TPR * i;
      kpv[i] = hpv[i] = 0.0;
      double v = 0.0;
      if (mo < M && t0 + n < N) {
        double r2 = 0.0;
#pragma unroll
        for (int q = 0; q < VB_MAXD; ++q) {
          if (q < d) {
            const double df = sh.z[mo][q] - sh.x[n][q];
            r2 = fma(df, df, r2);
          }
        }
        kprofile_grad<KID>(r2, kpv[i], hpv[i]);
        v = sf2 * kpv[i];
      }
      sh.u.tile.KT[n][mo] = v;
    }
    __syncthreads();
    vb_tile_mm<MP, VB_LOWER, false>(sh.u.tile.AT, sh.P, sh.u.tile.KT, nullptr, nullptr, 0.0);
    __syncthreads();
    if (tid < TN) {  // (A^T g)_n for g_s2's fifth term
      double s = 0.0;
      for (int m = 0; m < MP; ++m) s = fma(sh.u.tile.AT[tid][m], sh.g[m], s);
      pag = fma(s, s, pag);
    }
    vb_tile_mm<MP, VB_FULL, false>(sh.u.tile.KT, sh.Q, sh.u.tile.AT, sh.g, sh.y, rs4);
    __syncthreads();
    vb_tile_mm<MP, VB_UPPER, true>(sh.u.tile.AT, sh.P, sh.u.tile.KT, nullptr, nullptr, 0.0);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int n = co + TPR * i;
      if (mo < M && t0 + n < N) {
        const double kb = sh.u.tile.AT[n][mo];
        gsf = fma(kb, kpv[i], gsf);
        const double e1 = kb * (sf2 * hpv[i]);
#pragma unroll
        for (int q = 0; q < VB_MAXD; ++q) {
          if (q < d) {
            const double df = sh.z[mo][q] - sh.x[n][q];
            gls[q] = fma(e1 * df, df, gls[q]);
            gzz[q] = fma(e1, df, gzz[q]);
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- the sums: dF/dZ[mo] over the TPR lanes of a row, the rest over the workgroup ----
#pragma unroll
  for (int q = 0; q < VB_MAXD; ++q) {
    if (q < d) {
      double v = gzz[q];
#pragma unroll
      for (int o = TPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (a.gz && co == 0 && mo < M) a.gz[p * (int64_t)(M * d) + mo * d + q] = 2.0 * sh.ils[q] * v;
    }
  }
  const double agag = block_sum256(pag, sh.red);
  gsf = block_sum256(gsf, sh.red);
#pragma unroll
  for (int q = 0; q < VB_MAXD; ++q) {
    if (q < d) {
      const double v = block_sum256(gls[q], sh.red);
      if (tid == 0) out[1 + q] = -2.0 * sh.ils[q] * v;
    }
  }
  if (tid == 0) {
    const double s22 = s2 * s2, dM = (double)M;
    const double t0 = dN / (2.0 * s2), t1 = -(dM - trb) / (2.0 * s2), t2 = -yy / (2.0 * s22), t3 = ug / (s22 * s2);
    const double t4 = -agag / (2.0 * s22 * s22), t5 = -(kappa - sumA2) / (2.0 * s22);
    out[0] = F;
    out[1 + d] = gsf - dN / (2.0 * s2);
    out[2 + d] = -(t0 + t1 + t2 + t3 + t4 + t5);
    out[3 + d] = logmarg;
    out[4 + d] = trace;
    a.info[p] = 0;
  }
}

}  // namespace sgp
#endif  // __HIPCC__
