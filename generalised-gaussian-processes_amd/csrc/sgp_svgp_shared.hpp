// What the batched SVGP chains share: the theta-sample block, the K_uu / K_ub assembly, the triangle masks and the
// kernel-derivative contractions of sgp_svgp.hip's sgp_svgp_elbo_batch, moved here unchanged so that the multi-class chain
// (sgp_svgp_mc.hip: one theta, C classes in the batch index) runs the same code from Abar on.  Every launch carries the sample
// index in blockIdx.y.  The non-template kernels are `static`: each translation unit that includes this header has its own copy.
#pragma once
#include "sgp_dense.hpp"

namespace sgp {

static inline int grid_for_s(int64_t total, int cap = 2048) {
  int64_t g = (total + 255) / 256;
  if (g < 1) g = 1;
  return (int)(g < cap ? g : cap);
}

constexpr int SVGP_SPLITK = 16;  // k-slices of the two M x M x B products of the reverse pass

constexpr int SVGP_MAX_S = 8;
struct SvgpThetaS {  // a kernel argument (2.2 KB): theta never makes a host-to-device copy of its own
  KernArgs ka[SVGP_MAX_S];
  double s2[SVGP_MAX_S];
};

// Kp[s] = Kuu(theta_s) + jitter I, padded with the identity (the factorization's input), Mp x Mp
template <int KID>
// z_stride: doubles between the inducing inputs of consecutive samples (0: one Z for all of them)
__global__ __launch_bounds__(256) void svgp_kuu_batch_kernel(const double* __restrict__ Z, int64_t ldz, int64_t z_stride, SvgpThetaS th,
                                                             double jitter, int M, int Mp, double* __restrict__ Kp) {
  const KernArgs& ka = th.ka[blockIdx.y];
  Z += (int64_t)blockIdx.y * z_stride;
  double* K = Kp + (int64_t)blockIdx.y * Mp * Mp;
  const int64_t total = (int64_t)Mp * Mp;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e / Mp), j = (int)(e - (int64_t)i * Mp);
    double v = (i == j) ? 1.0 : 0.0;
    if (i < M && j < M) {
      double r2 = 0.0;
      for (int q = 0; q < ka.d; ++q) {
        const double df = (Z[i * ldz + q] - Z[j * ldz + q]) * ka.inv_ls[q];
        r2 = fma(df, df, r2);
      }
      v = ka.sf2 * kprofile<KID>(r2);
      if (i == j) v += jitter;
    }
    K[e] = v;
  }
}

template <int KID>
__global__ __launch_bounds__(256) void svgp_kub_batch_kernel(const double* __restrict__ Z, int64_t ldz, int64_t z_stride,
                                                             const double* __restrict__ Xb, int64_t ldx, SvgpThetaS th, int M, int Mp,
                                                             int B, int Bp, double* __restrict__ Kub) {
  const KernArgs& ka = th.ka[blockIdx.y];
  Z += (int64_t)blockIdx.y * z_stride;
  const int64_t total = (int64_t)Mp * Bp;
  double* K = Kub + (int64_t)blockIdx.y * total;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int m = (int)(e / Bp), b = (int)(e - (int64_t)m * Bp);
    double v = 0.0;
    if (m < M && b < B) {
      double r2 = 0.0;
      for (int q = 0; q < ka.d; ++q) {
        const double df = (Z[m * ldz + q] - Xb[b * ldx + q]) * ka.inv_ls[q];
        r2 = fma(df, df, r2);
      }
      v = ka.sf2 * kprofile<KID>(r2);
    }
    K[e] = v;
  }
}

static __global__ __launch_bounds__(256) void svgp_tril_batch_kernel(double* __restrict__ X, int Mp, double scale, int halve_diag) {
  const int64_t total = (int64_t)Mp * Mp;
  X += (int64_t)blockIdx.y * total;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int r = (int)(e / Mp), c = (int)(e - (int64_t)r * Mp);
    double v = X[e] * scale;
    if (c > r) v = 0.0;
    else if (c == r && halve_diag) v *= 0.5;
    X[e] = v;
  }
}

// Kernel-derivative contractions of sample blockIdx.y, one workgroup per inducing row and source:
//   blockIdx.x <  M : row m of Kubbar (Mp x Bp)   against d Kub[m][.]  (data = the minibatch rows)
//   blockIdx.x >= M : row m of sym(P) (Mp x Mp)   against d Kuu[m][.]  (data = the inducing inputs; Kuubar = (P + P^T) / 2)
// part[src][m][q] = sum E df_q^2 (q < d), part[src][m][d] = sum Kbar k', gz[src][m][q] = sum E df_q, E = Kbar sf2 dk'/dr2
template <int KID>
__global__ __launch_bounds__(256) void svgp_kbwd_batch_kernel(const double* __restrict__ Z, int64_t ldz, const double* __restrict__ Xb,
                                                              int64_t ldx, SvgpThetaS th, const double* __restrict__ Kbb,
                                                              const double* __restrict__ P, int M, int Mp, int Bp, int B,
                                                              double* __restrict__ part, double* __restrict__ gzraw) {
  __shared__ double red[4];
  const KernArgs& ka = th.ka[blockIdx.y];
  const int d = ka.d;
  const bool uu = (int)blockIdx.x >= M;
  const int m = uu ? (int)blockIdx.x - M : (int)blockIdx.x;
  const double* data = uu ? Z : Xb;
  const int64_t ldd = uu ? ldz : ldx;
  const int n = uu ? M : B;
  Kbb += (int64_t)blockIdx.y * Mp * Bp;
  P += (int64_t)blockIdx.y * Mp * Mp;
  part += ((int64_t)blockIdx.y * 2 + (uu ? 1 : 0)) * M * (d + 1);
  gzraw += ((int64_t)blockIdx.y * 2 + (uu ? 1 : 0)) * M * d;
  for (int q = 0; q <= d; ++q) {
    double s2 = 0.0, s1 = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) {
      double r2 = 0.0, dfq = 0.0;
      for (int j = 0; j < d; ++j) {
        const double df = (Z[m * ldz + j] - data[b * ldd + j]) * ka.inv_ls[j];
        r2 = fma(df, df, r2);
        if (j == q) dfq = df;
      }
      double kp, hp;
      kprofile_grad<KID>(r2, kp, hp);
      const double kb = uu ? 0.5 * (P[(int64_t)m * Mp + b] + P[(int64_t)b * Mp + m]) : Kbb[(int64_t)m * Bp + b];
      if (q == d) {
        s2 = fma(kb, kp, s2);
      } else {
        const double E = kb * ka.sf2 * hp;
        s1 = fma(E, dfq, s1);
        s2 = fma(E * dfq, dfq, s2);
      }
    }
    s2 = block_sum256(s2, red);
    s1 = block_sum256(s1, red);
    if (threadIdx.x == 0) {
      part[(size_t)m * (d + 1) + q] = s2;
      if (q < d) gzraw[(size_t)m * d + q] = s1;
    }
  }
}
// g_ls[s][q] = -2 inv_ls_q (sum_m part_ub + sum_m part_uu) ; g_sf2[s] = the two k' sums + sum_b dv / B ;
// g_Z[s][m][q] = inv_ls_q (2 gz_ub + 4 gz_uu): row AND column m of the symmetric Kuubar move with z_m
static __global__ __launch_bounds__(256) void svgp_kbwd_reduce_batch_kernel(const double* __restrict__ part, const double* __restrict__ gzraw,
                                                                            int M, SvgpThetaS th, const double* __restrict__ dv, int B, int Bp,
                                                                            double invB, double* g_ls, double* g_sf2, double* g_Z) {
  __shared__ double red[4];
  const KernArgs& ka = th.ka[blockIdx.y];
  const int d = ka.d;
  const double* pub = part + (int64_t)blockIdx.y * 2 * M * (d + 1);
  const double* puu = pub + (int64_t)M * (d + 1);
  const double* zub = gzraw + (int64_t)blockIdx.y * 2 * M * d;
  const double* zuu = zub + (int64_t)M * d;
  dv += (int64_t)blockIdx.y * Bp;
  if (blockIdx.x == 0) {
    for (int q = 0; q <= d; ++q) {
      double s = 0.0;
      for (int m = threadIdx.x; m < M; m += 256) s += pub[(size_t)m * (d + 1) + q] + puu[(size_t)m * (d + 1) + q];
      s = block_sum256(s, red);
      if (q == d) {
        double t = 0.0;
        for (int b = threadIdx.x; b < B; b += 256) t += dv[b];
        t = block_sum256(t, red);
        if (threadIdx.x == 0) g_sf2[blockIdx.y] = s + t * invB;
      } else if (threadIdx.x == 0) {
        g_ls[(int64_t)blockIdx.y * d + q] = -2.0 * ka.inv_ls[q] * s;
      }
    }
  }
  const int64_t total = (int64_t)M * d;
  double* gz = g_Z + (int64_t)blockIdx.y * total;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256)
    gz[e] = ka.inv_ls[(int)(e % d)] * (2.0 * zub[e] + 4.0 * zuu[e]);
}

}  // namespace sgp
