// The density of NUTS over the exact GP marginal likelihood in the unconstrained variables q = [log ls_1..d | log sig_f | log sig_n] --
// what targets.ExactHmcTarget applies around one evaluation (targets.in_range, _LogThetaTarget.constrain, theta_logp_and_grad(...,
// finite_grad=True)), restated for the device: priors ls ~ Gamma(2, 1), sig_f, sig_n ~ HalfCauchy(1), log-Jacobian sum q, chain rule
// d/d log v = v d/dv + 1.  One thread runs it between the evaluations of sgp_exact_nuts.hip; the same header compiles for the host
// (g++), where the CPU tests hold it against the Python functions operation by operation (the sums run left to right as Python's do).
#pragma once
#include <math.h>

#ifndef SGP_HD
#if defined(__HIPCC__)
#define SGP_HD __host__ __device__
#else
#define SGP_HD
#endif
#endif

namespace sgp {

constexpr int EXT_MAXD = 8;                           // lengthscales (EB_MAXD)
constexpr double EXT_Q_LIMIT = 300.0;                 // targets.in_range: exp() of the position must stay representable
constexpr double EXT_LOG_2_OVER_PI = -0.4515827052894549;  // log 2 - log pi

// targets.in_range: every entry finite and |q_i| < 300; outside it the density is zero and nothing is evaluated
SGP_HD inline bool ext_in_range(const double* q, int n) {
  for (int i = 0; i < n; ++i)
    if (!(isfinite(q[i]) && fabs(q[i]) < EXT_Q_LIMIT)) return false;
  return true;
}

// v = exp(q) = [ls_1..d | sig_f | sig_n], and the row the evaluation takes: theta = [ls_1..d | sig_f^2 | sig_n^2 + jitter]
SGP_HD inline void ext_constrain(const double* q, int d, double jitter, double* v, double* theta) {
  for (int i = 0; i < d + 2; ++i) v[i] = exp(q[i]);
  for (int i = 0; i < d; ++i) theta[i] = v[i];
  theta[d] = v[d] * v[d];
  theta[d + 1] = v[d + 1] * v[d + 1] + jitter;
}

// (F, g = [dF/dls_1..d | dF/dsf2 | dF/ds2], info) of the evaluation at v = exp(q) -> logp (returned) and grad[0..d+1] in q.  A non-zero
// info, a non-finite F or a non-finite gradient entry gives (-inf, zeros): a divergence for the sampler, never an error.
SGP_HD inline double ext_logp_grad(const double* q, const double* v, int d, double F, const double* g, int info, double* grad) {
  const int n = d + 2;
  bool ok = info == 0 && isfinite(F);
  double logp = -INFINITY;
  if (ok) {
    const double sf = v[d], sn = v[d + 1];
    double lp = 0.0, sq = 0.0;
    for (int j = 0; j < d; ++j) lp += log(v[j]) - v[j];
    lp += (EXT_LOG_2_OVER_PI - log1p(sf * sf)) + (EXT_LOG_2_OVER_PI - log1p(sn * sn));
    for (int j = 0; j < n; ++j) sq += q[j];
    logp = F + lp + sq;
    for (int j = 0; j < d; ++j) grad[j] = v[j] * (g[j] + (1.0 / v[j] - 1.0)) + 1.0;
    grad[d] = sf * (2.0 * sf * g[d] + -2.0 * sf / (1.0 + sf * sf)) + 1.0;
    grad[d + 1] = sn * (2.0 * sn * g[d + 1] + -2.0 * sn / (1.0 + sn * sn)) + 1.0;
    for (int j = 0; j < n; ++j) ok = ok && isfinite(grad[j]);
  }
  if (!ok) {
    for (int j = 0; j < n; ++j) grad[j] = 0.0;
    return -INFINITY;
  }
  return logp;
}

}  // namespace sgp
