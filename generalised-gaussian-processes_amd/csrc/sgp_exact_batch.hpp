// One exact-GP marginal likelihood (value + gradient) inside ONE 256-thread workgroup, the whole problem in that workgroup's LDS:
// the evaluation sgp_exact_eval_batch (sgp_exact_batch.hip: one problem per workgroup) and the batched device-resident NUTS
// (sgp_exact_nuts.hip: one chain per workgroup, one evaluation per leapfrog) share.  No inter-workgroup communication, no flags, no
// spins, no atomics.  eb_eval = eb_factor (A, L, u, the value) + eb_invert (L^-1, alpha, tr A^-1) + the gradient; the batched predictive
// (sgp_exact_predict.hip) runs the first two and goes on from L^-1 and alpha.
//
//   A = sf2 k'(X, X) + s2 I ; L = chol(A) ; u = L^-1 y ; F = -1/2 u.u - sum log L_ii - N/2 log 2 pi            (value-only stops here)
//   L^-1 in place ; alpha = L^-T u ; tr A^-1 = |L^-1|_F^2 ; G = alpha alpha^T - L^-T L^-1 (16 x 16 tiles, never stored)
//   dF/dls_q = 1/2 sum G dA/dls_q ; dF/dsf2 = 1/2 sum G k' ; dF/ds2 = 1/2 (alpha.alpha - tr A^-1)              (sgp_exact_eval's convention)
//
// The LDS image M is Nr x Nr (Nr = N rounded up to 16, identity in the padding) inside NP x (NP + 2) doubles, NP in {32, 64, 128} the
// size class: the layout of sgp_wg_dense.hpp (row stride, the two MFMA operand patterns, the row permutation `kperm` of eb_eval).  Row
// reads (assembly, alpha) are contiguous.  Every sum has a fixed order and depends on nothing outside the problem: the same bits on
// every call, stream and batch.
#pragma once
#include "sgp_common.hpp"
#include "sgp_wg_dense.hpp"

namespace sgp {

constexpr int EB_MAXN = 128;
constexpr int EB_MAXD = 8;
constexpr int64_t EB_MAXP = (1 << 24) - 1;  // one workgroup per problem: P x 256 work-items stay below the 2^32 of one launch
constexpr int EB_XLD = EB_MAXD + 1;  // odd stride: x_j reads of the epilogue (16 consecutive rows) hit distinct banks

template <int NP>
struct EbShared {
  double M[NP][NP + 2];
  double x[NP][EB_XLD];        // the data set's rows (unscaled: differences are formed first, then scaled)
  double yv[NP];               // y, then u = L^-1 y
  double al[NP];               // alpha
  double red[4][EB_MAXD + 2];  // block_sum256's four words / the waves' gradient partials
  int bad;
};

// (row, column) of entry t of a lower triangle stored row by row: t = r (r + 1) / 2 + c, c <= r
__device__ __forceinline__ void eb_tri(int t, int& r, int& c) {
  r = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f);
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  while (r * (r + 1) / 2 > t) --r;
  c = t - r * (r + 1) / 2;
}

// The size class of N
__host__ __device__ inline int eb_size_class(int N) { return N <= 32 ? 32 : (N <= 64 ? 64 : 128); }

// The data set's rows and its target into the workgroup's LDS (zero in the padding up to Nr = N rounded up to 16); `yv` is sh.yv or the
// caller's own copy of y (eb_eval overwrites sh.yv with u).  The caller synchronises (eb_eval's first barrier does).
template <int NP>
__device__ __forceinline__ void eb_load(EbShared<NP>& sh, double* yv, const double* __restrict__ Xp, int64_t ldx, const double* __restrict__ Yp,
                                        int N, int d) {
  const int tid = threadIdx.x, Nr = round_up(N, 16);
  for (int e = tid; e < Nr * d; e += 256) {
    const int i = e / d, q = e - i * d;
    sh.x[i][q] = i < N ? Xp[(int64_t)i * ldx + q] : 0.0;
  }
  for (int i = tid; i < Nr; i += 256) yv[i] = i < N ? Yp[i] : 0.0;
}

// What eb_factor leaves in registers (the same in every thread): F, u.u, sum log L_ii, and `bad` (0, or the 1-based first pivot at which
// A is not numerically positive definite -- 1 for a hyper-parameter that is not a positive finite number).
struct EbValue {
  double F, uu, ld;
  int bad;
};
// ... and eb_invert: tr A^-1 and alpha.alpha
struct EbInverse {
  double tr, aa;
};

// The value half of eb_eval, all 256 threads.  On entry sh.x holds the data set and sh.yv the target (eb_load; not yet synchronised),
// th = [ls_1..d | sf2 | s2].  Assembles A, factors it (sh.M = L, lower; sh.yv = u = L^-1 y) and returns the scalars of the value; ils
// receives 1 / ls_q (zero past d).  Ends on block_sum256's barrier.
template <int KID, int NP>
__device__ __forceinline__ EbValue eb_factor(EbShared<NP>& sh, const double* __restrict__ th, int N, int d, double (&ils)[EB_MAXD]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int Nr = round_up(N, 16), nb = Nr / 16;
  const double sf2 = th[d], s2 = th[d + 1];
#pragma unroll
  for (int q = 0; q < EB_MAXD; ++q) ils[q] = q < d ? 1.0 / th[q] : 0.0;
  if (tid == 0) {  // a hyper-parameter that is not a positive finite number (NaN included) is reported as pivot 1: 1 / ls loses a sign
    bool pos = true;
    for (int q = 0; q < d + 2; ++q) pos = pos && th[q] > 0.0 && th[q] < __builtin_inf();
    sh.bad = pos ? 0 : 1;
  }
  __syncthreads();

  // ---- A: lower triangle, zero above it, identity in the padding ----
  for (int e = tid; e < Nr * Nr; e += 256) {
    const int i = e / Nr, j = e - i * Nr;
    double v = 0.0;
    if (i < N && j <= i) {
      double r2 = 0.0;
#pragma unroll
      for (int q = 0; q < EB_MAXD; ++q) {
        if (q < d) {
          const double df = (sh.x[i][q] - sh.x[j][q]) * ils[q];
          r2 = fma(df, df, r2);
        }
      }
      v = sf2 * kprofile<KID>(r2);
      if (i == j) v += s2;
    } else if (i == j) {
      v = 1.0;
    }
    sh.M[i][j] = v;
  }
  __syncthreads();

  // ---- Cholesky, right-looking by 16-column panels, with the forward substitution of y carried along ----
  // A pivot at or below 8 N 2^-53 times the diagonal of A (sf2 + s2 in every row) is rounding noise of the updates that formed it: A is
  // not numerically positive definite.  The first such pivot is reported (1-based); the factorization continues on a unit pivot.
  const double gate = (sf2 + s2) * (8.0 * (double)N) * 0x1p-53;
  for (int pb = 0; pb < nb; ++pb) {
    const int c0 = 16 * pb;
    if (wave == 0) {  // (a) the 16 x 16 diagonal block: lane <-> row (the four lane groups hold copies), columns exchanged by shuffles
      double a[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) a[k] = sh.M[c0 + l15][c0 + k];
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        double dj = __shfl(a[jj], jj, 64);
        if (c0 + jj < N && !(dj > gate)) {  // (NaN included)
          if (lane == 0 && sh.bad == 0) sh.bad = c0 + jj + 1;
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
        for (int k = 0; k < 16; ++k) sh.M[c0 + l15][c0 + k] = (k <= l15) ? a[k] : 0.0;
      }
    }
    __syncthreads();
    const int nbelow = Nr - c0 - 16;
    if (tid < nbelow) {  // (b) the rows below: thread <-> row, x = row D^-T by substitution (the block's entries are broadcast reads)
      const int i = c0 + 16 + tid;
      double x[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) x[k] = sh.M[i][c0 + k];
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        double s = x[jj];
#pragma unroll
        for (int k = 0; k < jj; ++k) s = fma(-x[k], sh.M[c0 + jj][c0 + k], s);
        x[jj] = s / sh.M[c0 + jj][c0 + jj];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) sh.M[i][c0 + k] = x[k];
    }
    if (wave == 3) {  // ... and the block's 16 entries of u = L^-1 y
      double lrow[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) lrow[k] = sh.M[c0 + l15][c0 + k];
      double v = sh.yv[c0 + l15];
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const double xj = __shfl(v, jj, 64) / __shfl(lrow[jj], jj, 64);
        v = (l15 == jj) ? xj : (l15 > jj ? fma(-lrow[jj], xj, v) : v);
      }
      if (lane < 16) sh.yv[c0 + l15] = v;
    }
    __syncthreads();
    {  // (c) rank-16 update of the trailing lower-triangle tiles on the matrix cores; wave <-> tiles wave, wave + 4, ...
      const int m = nb - pb - 1;
      for (int t = wave; t < m * (m + 1) / 2; t += 4) {
        int ri, rj;
        eb_tri(t, ri, rj);
        const int i0 = 16 * (pb + 1 + ri), j0 = 16 * (pb + 1 + rj);
        d4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = sh.M[i0 + l4 + 4 * r][j0 + l15];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma16(-sh.M[i0 + l15][c0 + 4 * s + l4], sh.M[j0 + l15][c0 + 4 * s + l4], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) sh.M[i0 + l4 + 4 * r][j0 + l15] = acc[r];
      }
      if (tid < nbelow) {  // y below the block
        const int i = c0 + 16 + tid;
        double s = sh.yv[i];
#pragma unroll
        for (int k = 0; k < 16; ++k) s = fma(-sh.M[i][c0 + k], sh.yv[c0 + k], s);
        sh.yv[i] = s;
      }
    }
    __syncthreads();
  }

  // ---- the scalars of the value: one entry per thread, block_sum256's fixed tree ----
  double uu = 0.0, ld = 0.0;
  if (tid < N) {
    uu = sh.yv[tid] * sh.yv[tid];
    ld = log(sh.M[tid][tid]);
  }
  uu = block_sum256(uu, &sh.red[0][0]);
  ld = block_sum256(ld, &sh.red[0][0]);
  const int bad = sh.bad;
  const double F = -0.5 * uu - ld - 0.5 * (double)N * 1.8378770664093453;  // log 2 pi
  return EbValue{F, uu, ld, bad};
}

// The inverse, all 256 threads, after an eb_factor that returned bad == 0: sh.M = L^-1 in place (lower), sh.al = alpha = L^-T u (zero
// in the padding); sh.yv keeps u.  Ends on a barrier: sh.red is free again.
template <int NP>
__device__ __forceinline__ EbInverse eb_invert(EbShared<NP>& sh, int N) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int Nr = round_up(N, 16), nb = Nr / 16;

  // ---- L^-1 in place, block column by block column from the right:  Inv[below][J] = -Inv[below][below] L[below][J] Inv[J][J] ----
  for (int J = nb - 1; J >= 0; --J) {
    const int c0 = 16 * J, m = nb - 1 - J;
    d4 T[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {  // T = Inv[below][below] L[below][J]: every tile into registers before the panel is overwritten
      T[u] = d4{0.0, 0.0, 0.0, 0.0};
      const int ri = wave + 4 * u;
      if (ri < m) {
        const int i0 = 16 * (J + 1 + ri);
        for (int k0 = c0 + 16; k0 <= i0; k0 += 16) {
#pragma unroll
          for (int s = 0; s < 4; ++s) T[u] = mfma16(sh.M[i0 + l15][k0 + 4 * s + l4], sh.M[k0 + 4 * s + l4][c0 + l15], T[u]);
        }
      }
    }
    double xinv[16];  // wave 3, lane c < 16: column c of the inverse of the diagonal block (zero above the diagonal)
    if (wave == 3) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        double s = (r == l15) ? 1.0 : 0.0;
#pragma unroll
        for (int q = 0; q < r; ++q) s = fma(-sh.M[c0 + r][c0 + q], xinv[q], s);
        xinv[r] = s / sh.M[c0 + r][c0 + r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int ri = wave + 4 * u;
      if (ri < m) {
        const int i0 = 16 * (J + 1 + ri);
#pragma unroll
        for (int r = 0; r < 4; ++r) sh.M[i0 + l4 + 4 * r][c0 + l15] = T[u][r];
      }
    }
    if (wave == 3 && lane < 16) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sh.M[c0 + r][c0 + l15] = xinv[r];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {  // tile <- -T Inv[J][J]: a wave reads its own tile whole, then overwrites it
      const int ri = wave + 4 * u;
      if (ri < m) {
        const int i0 = 16 * (J + 1 + ri);
        double a[4], b[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          a[s] = -sh.M[i0 + l15][c0 + 4 * s + l4];
          b[s] = sh.M[c0 + 4 * s + l4][c0 + l15];
        }
        d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma16(a[s], b[s], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) sh.M[i0 + l4 + 4 * r][c0 + l15] = acc[r];
      }
    }
    __syncthreads();
  }

  // ---- alpha = L^-T u, tr A^-1 = |L^-1|_F^2 : thread <-> column ----
  double tr = 0.0, aa = 0.0;
  if (tid < Nr) {
    double s = 0.0, t = 0.0;
    for (int k = tid; k < Nr; ++k) {
      const double v = sh.M[k][tid];
      s = fma(v, sh.yv[k], s);
      t = fma(v, v, t);
    }
    sh.al[tid] = tid < N ? s : 0.0;
    if (tid < N) {
      tr = t;
      aa = s * s;
    }
  }
  tr = block_sum256(tr, &sh.red[0][0]);
  aa = block_sum256(aa, &sh.red[0][0]);
  __syncthreads();  // red is reused by the caller
  return EbInverse{tr, aa};
}

// All 256 threads of the workgroup.  On entry sh.x holds the data set and sh.yv the target (eb_load; not yet synchronised), th = [ls_1..d |
// sf2 | s2].  Writes out[0..3] = [F, y^T A^-1 y, log|A|, tr A^-1 (NaN without the gradient)], grads[0..d+1] (with_grad) and *info (0, or
// the 1-based first pivot at which A is not numerically positive definite; then out and grads are NaN).  th / out / grads / info may
// point to global memory or to LDS outside `sh`; they are written by threads 0..d+1 as the last thing, with no barrier after it.
template <int KID, int NP>
__device__ __forceinline__ void eb_eval(EbShared<NP>& sh, const double* __restrict__ th, int N, int d, int with_grad,
                                        double* __restrict__ out, double* __restrict__ grads, int* __restrict__ info) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int Nr = round_up(N, 16), nb = Nr / 16;
  const double sf2 = th[d];
  double ils[EB_MAXD];
  const EbValue val = eb_factor<KID, NP>(sh, th, N, d, ils);
  const int bad = val.bad;
  const double F = val.F, uu = val.uu, ld = val.ld;
  const double nan = __builtin_nan("");
  if (bad != 0 || !with_grad) {
    if (tid == 0) {
      out[0] = bad ? nan : F;
      out[1] = bad ? nan : uu;
      out[2] = bad ? nan : 2.0 * ld;
      out[3] = nan;
      *info = bad;
    }
    if (with_grad && tid < d + 2) grads[tid] = nan;
    return;
  }
  const EbInverse inv = eb_invert<NP>(sh, N);
  const double tr = inv.tr, aa = inv.aa;

  // ---- the lower-triangle 16 x 16 tiles of A^-1 = L^-T L^-1 on the matrix cores, each folded into the d + 1 sums at once ----
  double sq[EB_MAXD];
#pragma unroll
  for (int q = 0; q < EB_MAXD; ++q) sq[q] = 0.0;
  double sk = 0.0;
  const int kperm = 8 * (l4 & 1) + 4 * (l4 >> 1);  // see the head of sgp_wg_dense.hpp
  for (int t = wave; t < nb * (nb + 1) / 2; t += 4) {
    int bi, bj;
    eb_tri(t, bi, bj);
    const int i0 = 16 * bi, j0 = 16 * bj;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = i0; k0 < Nr; k0 += 16) {  // (A^-1)_ij = sum_{k >= max(i, j)} (L^-1)_ki (L^-1)_kj : the zeros above are never multiplied
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double* row = &sh.M[k0 + kperm + s][0];
        acc = mfma16(row[i0 + l15], row[j0 + l15], acc);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // element r of the accumulator: row (lane >> 4) + 4 r, column lane & 15
      const int li = l4 + 4 * r, gi = i0 + li, gj = j0 + l15;
      double w = (bi == bj) ? (li > l15 ? 2.0 : (li == l15 ? 1.0 : 0.0)) : 2.0;
      if (gi >= N || gj >= N) w = 0.0;
      const double g = w * fma(sh.al[gi], sh.al[gj], -acc[r]);
      double r2 = 0.0;
#pragma unroll
      for (int q = 0; q < EB_MAXD; ++q) {
        if (q < d) {
          const double df = (sh.x[gi][q] - sh.x[gj][q]) * ils[q];
          r2 = fma(df, df, r2);
        }
      }
      double kp, hp;
      kprofile_grad<KID>(r2, kp, hp);
      sk = fma(g, kp, sk);
      const double e = g * hp;
#pragma unroll
      for (int q = 0; q < EB_MAXD; ++q) {
        if (q < d) {
          const double df = (sh.x[gi][q] - sh.x[gj][q]) * ils[q];
          sq[q] = fma(e * df, df, sq[q]);
        }
      }
    }
  }
  sk = wave_sum(sk);
  if (lane == 0) sh.red[wave][d] = sk;
#pragma unroll
  for (int q = 0; q < EB_MAXD; ++q) {
    if (q < d) {
      const double a = wave_sum(sq[q]);
      if (lane == 0) sh.red[wave][q] = a;
    }
  }
  __syncthreads();
  if (tid <= d) {
    const double s = (sh.red[0][tid] + sh.red[1][tid]) + (sh.red[2][tid] + sh.red[3][tid]);
    grads[tid] = tid == d ? 0.5 * s : -sf2 * (1.0 / th[tid]) * s;
  }
  if (tid == 0) {
    grads[d + 1] = 0.5 * (aa - tr);
    out[0] = F;
    out[1] = uu;
    out[2] = 2.0 * ld;
    out[3] = tr;
    *info = 0;
  }
}

}  // namespace sgp
