// Host build of the wide device sampler (csrc/sgp_nuts_wide.hpp) for the CPU tests: the state machine the joint kernel runs,
// driven by a log-density supplied as a C callback (ctypes) and checked draw for draw against hmc.NUTS.
#include <vector>

#include "sgp_nuts_wide.hpp"

extern "C" {
typedef void (*logp_cb)(const double* q, double* logp, double* grad);

long nuts_wide_host_run(int ndim, int n_tune, int n_draws, int max_treedepth, double step_scale, double target_accept,
                        unsigned long long seed, const double* q0, logp_cb cb, double* samples, double* stats) {
  static sgp::WideState s;
  std::vector<double> ws(sgp::wide_ws_doubles(ndim)), qpub(ndim), grad(ndim);
  const sgp::WideWs w = sgp::wide_ws_carve(ws.data(), ndim);
  sgp::wnuts_init(s, w, 0, ndim, n_tune, n_draws, max_treedepth, step_scale, target_accept, seed, q0);
  double lp = 0.0;
  for (;;) {
    const int cmd = sgp::wnuts_step(s, w, 0, lp, grad.data(), qpub.data(), samples, stats);
    if (s.slot_overflow) return -2;
    if (cmd == sgp::NUTS_DONE) break;
    cb(qpub.data(), &lp, grad.data());
  }
  if (s.slot_overflow) return -2;  // the slot pool ran out (wn_alloc)
  int held = 0;  // only the current state may still hold a slot
  for (int k = 0; k < sgp::WN_SLOTS; ++k) held += s.refc[k];
  return held == 1 && s.refc[s.s_cur] == 1 ? s.n_leapfrog : -1;
}
}

#ifdef NUTS_HOST_MAIN
// Sanitizer build (tests/test_all_in_hmc.py): Gaussians from 1 to 3 098 dimensions, a zero-density wall (divergences), tree-depth
// limits 1 and 10; the slot pool must come back empty after every draw.
#include <cmath>
#include <cstdio>
static int g_ndim = 1;
static int g_wall = 0;
static void target(const double* q, double* logp, double* grad) {
  double lp = 0.0;
  for (int i = 0; i < g_ndim; ++i) {
    const double sd = 0.2 + 0.3 * (i % 7);
    const double z = (q[i] - 0.01 * i) / sd;
    lp -= 0.5 * z * z;
    grad[i] = -z / sd;
  }
  if (g_wall && q[0] > 0.7) lp = -INFINITY;
  *logp = lp;
}
int main() {
  long total = 0;
  for (int ndim : {1, 2, 257, 3098})
    for (int wall = 0; wall < 2; ++wall)
      for (int depth : {1, 10}) {
        g_ndim = ndim;
        g_wall = wall;
        const int tune = 30, draws = 20;
        std::vector<double> q0(ndim, 0.1), samples((size_t)draws * ndim), stats((size_t)draws * 8);
        const long nl = nuts_wide_host_run(ndim, tune, draws, depth, 0.25, 0.8, 99ull + ndim, q0.data(), target, samples.data(), stats.data());
        if (nl < 0) return 3;
        total += nl;
        for (double v : samples)
          if (!std::isfinite(v)) return 2;
      }
  std::printf("sanitized wide sampler ok %ld\n", total);
  return 0;
}
#endif
