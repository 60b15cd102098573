// The predictive of one collapsed (Titsias / VFE) sparse GP inside ONE 256-thread workgroup: the evaluation of sgp_vfe_predict_batch
// (sgp_vfe_predict.hip, include/sgp_vfe_predict.h: one problem per workgroup).  No inter-workgroup communication, no flags, no spins,
// no atomics.  With sgp_vfe_batch.hpp's notation (K = sf2 k'(Z, Z) + J I, L = chol K, A = L^-1 K_uf, B = I + A A^T / s2, L_B = chol B,
// u = A y, g = B^-1 u) the predictive sgp_predict documents in include/sgp.h is, per test point t,
//
//   a*_t = L^-1 k_u*(t) ;  v_t = L_B^-1 a*_t ;  mean_t = a*_t^T g / s2 ;  var_t = sf2 - sum_m a*_mt^2 + sum_m v_mt^2  (+ s2)
//
// The variance.  It is reported as it comes out of  ((sf2 - sum a*^2) + sum v^2) + s2 : it is NOT clamped, as in
// sgp_exact_predict_batch (sgp_exact_predict.hpp).  With pred_noise = 0 at a test point that coincides with an inducing input the
// result is rounding noise around s2-sized values and, for tiny s2, may be a small negative number; a clamp would hide by how much the
// subtraction cancelled, and the mixture over draws needs no positivity of the latent variance for its two moments.
//
// Two stages.
//   vp_train : everything vb_eval (sgp_vfe_batch.hpp) does up to and including its value scalars -- the theta check, the scaled
//              coordinates, K, vb_chol, vb_invert, pass 1 over the row tiles, chol B, L_B^-1, c0, g, F / logmarg / trace.  It is a COPY
//              of those lines of vb_eval, operation for operation in the same order, so that F has the bits of sgp_vfe_eval_batch's
//              out[p][0] (tests/test_vfe_predict_gpu.py holds it to that).  Cutting vb_eval itself into stages changed the machine code
//              of sgp_vfe_batch.hip and sgp_vfe_nuts.hip, so vb_eval stays as it is: A FIX TO EITHER COPY HAS TO BE MADE
//              IN THE OTHER AS WELL.  It leaves sh.P = L^-1, sh.Q = L_B^-1, sh.g = g, sh.z and sh.ils.
//   vp_test  : per tile of TN = vb_tile_rows(Mp) test points (128 / 64 / 32), in the LDS bytes of the row tiles (sh.x, u.tile.KT,
//              u.tile.AT): the scaled test rows, KT[n][m] = sf2 k' (zero for m >= M and t >= T), AT = P KT on the matrix cores
//              (vb_tile_mm, clipped to L^-1's triangle), mean and sum a*^2 from AT, KT <- Q AT (V, in the bytes of the dead K tile),
//              sum v^2 from KT.  The sums over m of a test point run over 256 / TN = Mp / 8 neighbouring lanes, lane j the entries
//              j, j + Mp / 8, ... (8 of them, in that order), then a fixed butterfly: every order depends on M's class alone, and a
//              test point's slot in its tile on t alone -- mean[t] and var[t] have the same bits for every T, P, stream and grid.
// No LDS beyond VbShared<MP>.
//
// The first part of this header is plain C++ (limits, the shape check, the workspace): a host program can include it without HIP
// (tests/native/vfe_predict_host.cpp).
#pragma once
#include "sgp_vfe_batch.hpp"

namespace sgp {

constexpr int64_t VP_MAXT = 32768;  // sgp_predict's and sgp_exact_predict_batch's limit on T

// SGP_OK, or what the entry points refuse a shape with: SGP_ERR_ARG before SGP_ERR_DIM (vb_check's rules plus T)
SGP_VB_HD inline int vp_check(int64_t P, int64_t N, int M, int d, int64_t T, int kernel_id) {
  if (T <= 0) return SGP_ERR_ARG;
  const int chk = vb_check(P, N, M, d, kernel_id);
  if (chk != SGP_OK) return chk;
  return T > VP_MAXT ? SGP_ERR_DIM : SGP_OK;
}

// The workspace: the family's placeholder unit (the problem lives in its workgroup's LDS; the kernel never touches the buffer)
SGP_VB_HD inline size_t vp_workspace_bytes(int64_t P, int64_t N, int M, int d, int64_t T) {
  return vp_check(P, N, M, d, T, 0) == SGP_OK ? VB_WS_UNIT : 0;
}

}  // namespace sgp

#if defined(__HIPCC__)

namespace sgp {

struct VpArgs {
  const double *X, *Y, *Z, *Xs, *theta;
  int64_t x_stride, ldx, y_stride, z_stride, ldz, xs_stride, ldxs;
  const int *ix, *iy, *iz, *ixs;
  int N, M, d, T, pred_noise;
  double jitter;
  double *mean, *var, *bound;
  int* info;
};

// What the training stage leaves in registers (every thread holds the same values)
struct VpTrain {
  double sf2, s2, F;
};

// The training stage: vb_eval's lines up to its value scalars (see the head of this file: a copy, keep the two in step).  Returns 0,
// or the `info` of the failure (uniform over the workgroup; nothing has been written to global memory).
template <int KID, int MP>
__device__ __forceinline__ int vp_train(VbShared<MP>& sh, const double* __restrict__ Xp, int64_t ldx, const double* __restrict__ Yp,
                                        const double* __restrict__ Zp, int64_t ldz, const double* __restrict__ th, int N, int M, int d,
                                        double jitter, VpTrain& tr) {
  constexpr int TN = vb_tile_rows(MP), TPR = vb_threads_per_row(MP), NI = MP / 16, NE = 8;
  constexpr int NACC = NI == 4 ? 4 : 1;
  static_assert(TN * MP == 256 * NE && MP / TPR * TPR == MP, "8 entries per thread");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int n_tiles = vb_tiles(N, MP);
  const int mo = tid / TPR, co = tid % TPR;  // this thread's inducing input and column class

  if (tid == 0) sh.bad = vb_theta_ok(th, d + 2) ? 0 : 1;
  if (tid < VB_MAXD) sh.ils[tid] = tid < d ? 1.0 / th[tid] : 0.0;
  for (int e = tid; e < MP * d; e += 256) {
    const int i = e / d, q = e - i * d;
    sh.z[i][q] = i < M ? Zp[(int64_t)i * ldz + q] * (1.0 / th[q]) : 0.0;
  }
  __syncthreads();
  if (sh.bad != 0) return sh.bad;  // (uniform over the workgroup)
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
      if (i == j) v += jitter;
    } else if (i == j) {
      v = 1.0;
    }
    sh.P[i][j] = v;
  }
  __syncthreads();
  // A pivot at or below 8 M 2^-53 times the diagonal of K is rounding noise of the updates that formed it
  vb_chol<MP>(sh.P, M, (sf2 + jitter) * (8.0 * (double)M) * 0x1p-53, 0, &sh.bad);
  if (sh.bad != 0) return sh.bad;
  vb_invert<MP>(sh.P);

  // ---- pass 1: A_t = L^-1 K_uf,t ; A A^T ; u = A y ; sum A o A ; y.y ----
  d4 acc[NACC];
#pragma unroll
  for (int q = 0; q < NACC; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
  double pu = 0.0, pa2 = 0.0, pyy = 0.0;
  const int kperm = 8 * (l4 & 1) + 4 * (l4 >> 1);  // both operands of A A^T run down a column: sgp_wg_dense.hpp's row permutation
  for (int it = 0; it < n_tiles; ++it) {
    const int t0 = it * TN;
    vb_load_rows<MP>(sh, Xp, ldx, Yp, t0, N, d);
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
  if (sh.bad != 0) return sh.bad;
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
  tr.sf2 = sf2, tr.s2 = s2, tr.F = logmarg - trace;
  return 0;
}

// sum over m of f(T[n][m]) for the test point n = tid / (Mp / 8): lane j = tid % (Mp / 8) takes m = j, j + Mp / 8, ... in that order,
// the Mp / 8 partial sums meet in a fixed butterfly (every lane of the group ends with the total)
template <int MP>
__device__ __forceinline__ void vp_point_sums(const double (*Tl)[MP + 2], const double* gv, double& dot, double& sq) {
  constexpr int TPP = MP / 8;
  const int n = threadIdx.x / TPP, j = threadIdx.x % TPP;
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double v = Tl[n][j + TPP * i];
    if (gv) s = fma(v, gv[j + TPP * i], s);
    q = fma(v, v, q);
  }
#pragma unroll
  for (int o = TPP / 2; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  dot = s, sq = q;
}

// The test stage (the head of this file).  sh.P = L^-1, sh.Q = L_B^-1, sh.g, sh.z, sh.ils as vp_train left them.
template <int KID, int MP>
__device__ __forceinline__ void vp_test(VbShared<MP>& sh, const double* __restrict__ Xsp, int64_t ldxs, int T, int M, int d, double sf2,
                                        double s2, double noise, double* __restrict__ mean, double* __restrict__ var) {
  constexpr int TN = vb_tile_rows(MP), TPR = vb_threads_per_row(MP), NE = 8, TPP = MP / 8;
  static_assert(TPP * TN == 256, "Mp / 8 lanes per test point");
  const int tid = threadIdx.x;
  const int mo = tid / TPR, co = tid % TPR;
  const int pn = tid / TPP, pj = tid % TPP;  // the test point of the tile whose sums this thread shares in, and its lane among them
  __syncthreads();  // the bytes of B (u.mid.S) become the tiles again; sh.g is complete
  for (int t0 = 0; t0 < T; t0 += TN) {
    for (int e = tid; e < TN * d; e += 256) {
      const int n = e / d, q = e - n * d;
      sh.x[n][q] = t0 + n < T ? Xsp[(int64_t)(t0 + n) * ldxs + q] * sh.ils[q] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int n = co + TPR * i;
      double v = 0.0;
      if (mo < M && t0 + n < T) {
        double r2 = 0.0;
#pragma unroll
        for (int q = 0; q < VB_MAXD; ++q) {
          if (q < d) {
            const double df = sh.z[mo][q] - sh.x[n][q];
            r2 = fma(df, df, r2);
          }
        }
        double kp, hp;
        kprofile_grad<KID>(r2, kp, hp);  // (the profile of pass 1: a test point on a training row gets that row's k_uf bits)
        v = sf2 * kp;
      }
      sh.u.tile.KT[n][mo] = v;
    }
    __syncthreads();
    vb_tile_mm<MP, VB_LOWER, false>(sh.u.tile.AT, sh.P, sh.u.tile.KT, nullptr, nullptr, 0.0);  // a* = L^-1 k_u*
    __syncthreads();
    double ag, a2, unused, v2;
    vp_point_sums<MP>(sh.u.tile.AT, sh.g, ag, a2);
    vb_tile_mm<MP, VB_LOWER, false>(sh.u.tile.KT, sh.Q, sh.u.tile.AT, nullptr, nullptr, 0.0);  // v = L_B^-1 a*, over the dead K tile
    __syncthreads();
    vp_point_sums<MP>(sh.u.tile.KT, nullptr, unused, v2);
    if (pj == 0 && t0 + pn < T) {
      mean[t0 + pn] = ag / s2;
      var[t0 + pn] = ((sf2 - a2) + v2) + noise;
    }
    // (the next tile's KT is written after the barrier that follows its row load: these reads of KT are done by then)
  }
}

template <int KID, int MP>
__device__ __forceinline__ void vp_eval(VbShared<MP>& sh, const VpArgs& a, int64_t p) {
  const int tid = threadIdx.x;
  const int N = a.N, M = a.M, d = a.d, T = a.T;
  const double* Xp = a.X + (int64_t)(a.ix ? a.ix[p] : 0) * a.x_stride;
  const double* Yp = a.Y + (int64_t)(a.iy ? a.iy[p] : 0) * a.y_stride;
  const double* Zp = a.Z + (int64_t)(a.iz ? a.iz[p] : 0) * a.z_stride;
  const double* Xsp = a.Xs + (int64_t)(a.ixs ? a.ixs[p] : 0) * a.xs_stride;
  const double* th = a.theta + p * (d + 2);
  double* mean = a.mean + p * (int64_t)T;
  double* var = a.var + p * (int64_t)T;

  VpTrain tr;
  const int bad = vp_train<KID, MP>(sh, Xp, a.ldx, Yp, Zp, a.ldz, th, N, M, d, a.jitter, tr);
  if (bad != 0) {  // (uniform over the workgroup)
    const double nan = __builtin_nan("");
    for (int t = tid; t < T; t += 256) {
      mean[t] = nan;
      var[t] = nan;
    }
    if (tid == 0) {
      if (a.bound) a.bound[p] = nan;
      a.info[p] = bad;
    }
    return;
  }
  vp_test<KID, MP>(sh, Xsp, a.ldxs, T, M, d, tr.sf2, tr.s2, a.pred_noise ? tr.s2 : 0.0, mean, var);
  if (tid == 0) {
    if (a.bound) a.bound[p] = tr.F;
    a.info[p] = 0;
  }
}

}  // namespace sgp
#endif  // __HIPCC__
