// Host build of csrc/sgp_exact_target.hpp for tests/test_exact_nuts.py: the density transform the device sampler applies around one
// evaluation, callable through ctypes so that it can be held against targets.theta_logp_and_grad.
#include "sgp_exact_target.hpp"

extern "C" {

int ext_host_in_range(const double* q, int n) { return sgp::ext_in_range(q, n) ? 1 : 0; }

// v (d + 2) and theta (d + 2) out
void ext_host_constrain(const double* q, int d, double jitter, double* v, double* theta) { sgp::ext_constrain(q, d, jitter, v, theta); }

// the whole of ExactHmcTarget._eval after the evaluation: returns logp, fills grad (d + 2)
double ext_host_logp_grad(const double* q, int d, double F, const double* g, int info, double* grad) {
  double v[sgp::EXT_MAXD + 2], theta[sgp::EXT_MAXD + 2];
  sgp::ext_constrain(q, d, 0.0, v, theta);
  return sgp::ext_logp_grad(q, v, d, F, g, info, grad);
}
}
