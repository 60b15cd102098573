// The batched exact-GP predictive (sgp_exact_predict.hip): what one test point contributes to the mixture over the draws of a group, as
// plain C++ that a host program can run (tests/native/exact_mixture_host.cpp), and the limits of the two entry points.  This header
// includes nothing of HIP: the kernels' own code (the LDS image, the matrix-core product) lives in the .hip file.
//
// The variance.  sgp_exact_predict (sgp_exact.hip) reports var = sf2 - sum_i V_it^2 (+ s2) as it comes out of the subtraction: it does
// NOT clamp.  At a test point that coincides with a training point and with pred_noise = 0 the result is rounding noise around zero
// and may be a small negative number.  The batched kernel does the same, for the same reason: a clamp would hide by how much the
// subtraction cancelled, and the mixture over draws needs no positivity of the latent variance for its two moments.  The density
// outputs of the mixture do: a kept draw whose variance is not positive gives NaN there (log of a non-positive number), at that test
// point alone.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SGP_EP_HD __host__ __device__
#else
#define SGP_EP_HD
#endif

namespace sgp {

constexpr int64_t EP_MAXT = 32768;  // sgp_exact_predict's limit on T
constexpr int EP_TILE = 16;         // test points per tile of the predictive kernel

// log N(y | mu, v)
SGP_EP_HD inline double ep_logdens(double y, double mu, double v) {
  const double dlt = y - mu;
  const double q = 0.5 * (dlt * dlt) / v;
  return -0.5 * log(6.283185307179586 * v) - q;
}

struct EpMixPoint {
  double mean, var, logpdf, mean_logpdf;
  int64_t kept;
};

// One (group, test point): the draws are entries 0, stride, 2 stride, ... (n_draws of them) of mean / var, with info[s] per draw; a
// draw with info != 0 is skipped.  Serial, in index order, every sum from zero:
//   mean = (1/n) sum mu_s ; var = (1/n) sum (v_s + (mu_s - mean)^2)  (second pass, not E[x^2] - E[x]^2)
//   with y (has_y): l_s = log N(y | mu_s, v_s) ; logpdf = log((1/n) sum exp l_s) = max l + log((sum exp(l_s - max l)) / n) ;
//   mean_logpdf = (1/n) sum l_s.
// n = 0: every output is NaN (kept = 0).  Without y the two density outputs are NaN here and the kernel does not write them.
SGP_EP_HD inline EpMixPoint ep_mix_point(const double* mean, const double* var, const int* info, int64_t n_draws, int64_t stride,
                                         int has_y, double y) {
  EpMixPoint r;
  const double nan = NAN;
  int64_t n = 0;
  double sm = 0.0;
  for (int64_t s = 0; s < n_draws; ++s) {
    if (info[s] != 0) continue;
    ++n;
    sm += mean[s * stride];
  }
  r.kept = n;
  r.mean = r.var = r.logpdf = r.mean_logpdf = nan;
  if (n == 0) return r;
  const double dn = (double)n;
  const double m = sm / dn;
  double sv = 0.0, mx = -INFINITY, sl = 0.0;
  bool any_nan = false;
  for (int64_t s = 0; s < n_draws; ++s) {  // the second pass: the variance and, with y, the largest and the sum of the log densities
    if (info[s] != 0) continue;
    const double mu = mean[s * stride], v = var[s * stride];
    const double dlt = mu - m;
    sv += v + dlt * dlt;
    if (has_y) {
      const double l = ep_logdens(y, mu, v);
      any_nan = any_nan || l != l;
      mx = l > mx ? l : mx;
      sl += l;
    }
  }
  r.mean = m;
  r.var = sv / dn;
  if (!has_y) return r;
  r.mean_logpdf = sl / dn;
  if (any_nan) {
    r.logpdf = nan;
  } else if (mx == -INFINITY) {  // every density is zero
    r.logpdf = -INFINITY;
  } else {
    double se = 0.0;
    for (int64_t s = 0; s < n_draws; ++s) {
      if (info[s] != 0) continue;
      se += exp(ep_logdens(y, mean[s * stride], var[s * stride]) - mx);
    }
    r.logpdf = mx + log(se / dn);
  }
  return r;
}

}  // namespace sgp
