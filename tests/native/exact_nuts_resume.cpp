// Stand-alone host check of the resumable chain of csrc/sgp_exact_nuts.hip (tests/test_exact_nuts.py builds it with
// -fsanitize=address,undefined and runs it): nuts_step + the density transform of sgp_exact_target.hpp drive 50 draws on a Gaussian
// stand-in for the marginal likelihood, once straight through and once with the chain -- the sampler's state and the last (logp,
// gradient) -- copied with memcpy into fresh storage every 3 evaluations, the old storage poisoned and freed, and the run resumed
// from the copy, as a launch of the device sampler resumes from the workspace.  Both runs must print the same bytes.
//
//   exact_nuts_resume <chunk>      chunk = 0: straight through; chunk = k > 0: save / resume every k evaluations
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sgp_exact_target.hpp"
#include "sgp_nuts.hpp"

namespace {

constexpr int D = 3, ND = D + 2;

struct Chain {  // what the device keeps per chain between launches
  sgp::NutsState st;
  double lp, grad[ND];
};

// F(ls, sf2, s2) = -1/2 sum_i (theta_i - m_i)^2 / w_i over the evaluation's row theta = [ls | sf2 | s2], and dF/dtheta
void stand_in(const double* theta, double* F, double* g) {
  const double m[ND] = {1.5, 0.7, 2.0, 1.2, 0.3}, w[ND] = {0.5, 0.2, 1.0, 0.4, 0.1};
  double s = 0.0;
  for (int i = 0; i < ND; ++i) {
    const double r = theta[i] - m[i];
    s += r * r / w[i];
    g[i] = -r / w[i];
  }
  *F = -0.5 * s;
}

}  // namespace

int main(int argc, char** argv) {
  const int chunk = argc > 1 ? atoi(argv[1]) : 0;
  const int n_tune = 30, n_draws = 50;
  const double q0[ND] = {0.2, -0.1, 0.4, 0.1, -0.6};
  double* samples = (double*)malloc(sizeof(double) * n_draws * ND);
  double* stats = (double*)malloc(sizeof(double) * n_draws * sgp::NST_COLS);
  Chain* ch = (Chain*)malloc(sizeof(Chain));
  memset(ch, 0, sizeof(Chain));
  sgp::nuts_init(ch->st, ND, n_tune, n_draws, 6, 0.25, 0.8, 0x1234abcdULL, q0);
  long evals = 0, resumes = 0;
  for (;;) {
    const double* qn = nullptr;
    if (sgp::nuts_step(ch->st, ch->lp, ch->grad, &qn, samples, stats) != sgp::NUTS_EVAL) break;
    if (!sgp::ext_in_range(qn, ND)) {
      ch->lp = -INFINITY;
      for (int i = 0; i < ND; ++i) ch->grad[i] = 0.0;
    } else {
      double q[ND], v[ND], theta[ND], F, g[ND];
      for (int i = 0; i < ND; ++i) q[i] = qn[i];
      sgp::ext_constrain(q, D, 1e-6, v, theta);
      stand_in(theta, &F, g);
      ch->lp = sgp::ext_logp_grad(q, v, D, F, g, 0, ch->grad);
    }
    ++evals;
    if (chunk > 0 && evals % chunk == 0) {  // the launch ends here: the next one sees nothing but the copy
      Chain* next = (Chain*)malloc(sizeof(Chain));
      memcpy(next, ch, sizeof(Chain));
      memset(ch, 0xA5, sizeof(Chain));
      free(ch);
      ch = next;
      ++resumes;
    }
  }
  fprintf(stderr, "evaluations %ld, resumes %ld\n", evals, resumes);
  printf("evaluations %ld draws %d\n", (long)ch->st.n_leapfrog, ch->st.it);
  for (int r = 0; r < n_draws; ++r) {
    for (int i = 0; i < ND; ++i) printf("%a ", samples[r * ND + i]);
    for (int i = 0; i < sgp::NST_COLS; ++i) printf("%a ", stats[r * sgp::NST_COLS + i]);
    printf("\n");
  }
  free(ch);
  free(samples);
  free(stats);
  return 0;
}
