// Stand-alone host program: the per-point arithmetic of the mixture quantiles (csrc/sgp_mixture.hpp: mq_point) on cases read from a
// text file, and beside it an 80-bit restatement (erfcl, bisection to a fixed point) as the control of the acceptance rule.  Results are
// printed as hexadecimal floats.  Built by g++ alone (tests/test_mixture_quantile.py builds it with AddressSanitizer + UBSan); nothing
// of HIP is needed.
//
// Input:  G T P Q has_y / probs[Q] / offsets[G + 1] / info[P] / mean[P x T] / var[P x T] / y[G x T] (has_y)
// Output: one line per (g, t):  g t iters pit quant[Q] control[Q]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sgp_mixture.hpp"

static bool read_doubles(FILE* f, std::vector<double>& v) {
  for (double& x : v) {
    char tok[64];
    if (fscanf(f, "%63s", tok) != 1) return false;
    x = strtod(tok, nullptr);
  }
  return true;
}

// The quantile in long double: the tail sum with erfcl, bisection over the same proven bracket until the midpoint no longer moves.
static double control(const double* mean, const double* var, const int* info, long long n_draws, long long stride, double p_tail, int upper) {
  long double lo = INFINITY, hi = -INFINITY;
  long long n = 0;
  const long double z = sqrtl(-2.0L * logl((long double)p_tail));
  for (long long s = 0; s < n_draws; ++s) {
    if (info[s] != 0) continue;
    ++n;
    const long double mu = mean[s * stride], v = var[s * stride];
    if (!(v > 0.0L) || !(v < INFINITY) || !(fabsl(mu) < INFINITY)) return NAN;
    const long double sg = sqrtl(v);
    lo = fminl(lo, mu - 2.0L * z * sg);
    hi = fmaxl(hi, mu + 2.0L * z * sg);
  }
  if (n == 0) return NAN;
  for (int it = 0; it < 20000; ++it) {
    const long double mid = lo + 0.5L * (hi - lo);
    if (mid <= lo || mid >= hi) return (double)mid;
    long double sum = 0.0L;
    for (long long s = 0; s < n_draws; ++s) {
      if (info[s] != 0) continue;
      const long double u = (mid - (long double)mean[s * stride]) / (sqrtl((long double)var[s * stride]) * sqrtl(2.0L));
      sum += 0.5L * erfcl(upper ? u : -u);
    }
    const long double tail = sum / (long double)n;
    const bool above = upper ? tail > (long double)p_tail : tail < (long double)p_tail;
    if (above) lo = mid; else hi = mid;
  }
  return NAN;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  long long G, T, P;
  int Q, has_y;
  if (fscanf(f, "%lld %lld %lld %d %d", &G, &T, &P, &Q, &has_y) != 5 || G < 1 || T < 1 || P < 0 || Q < 1 || Q > sgp::MQ_MAXQ) return 2;
  std::vector<double> probs(Q);
  if (!read_doubles(f, probs)) return 2;
  std::vector<long long> off(G + 1);
  for (long long& o : off)
    if (fscanf(f, "%lld", &o) != 1) return 2;
  std::vector<int> info(P);
  for (int& i : info)
    if (fscanf(f, "%d", &i) != 1) return 2;
  std::vector<double> mean(P * T), var(P * T), y(has_y ? G * T : 0);
  if (!read_doubles(f, mean) || !read_doubles(f, var) || !read_doubles(f, y)) return 2;
  fclose(f);
  if (off[0] != 0 || off[G] != P) return 2;
  sgp::MqProbs pr{};
  for (int q = 0; q < sgp::MQ_MAXQ; ++q) pr.p_tail[q] = 0.5;
  for (int q = 0; q < Q; ++q) {
    if (!sgp::mq_prob_ok(probs[q])) return 2;
    sgp::mq_split(probs[q], &pr.p_tail[q], &pr.upper[q]);
  }
  for (long long g = 0; g < G; ++g) {
    if (off[g + 1] < off[g]) return 2;
    for (long long t = 0; t < T; ++t) {
      const long long s0 = off[g];
      double quant[sgp::MQ_MAXQ], pit;
      int iters;
      sgp::mq_point<sgp::MQ_MAXQ>(mean.data() + s0 * T + t, var.data() + s0 * T + t, info.data() + s0, off[g + 1] - s0, T, Q, pr, has_y,
                                  has_y ? y[g * T + t] : 0.0, quant, &pit, &iters);
      if (Q <= 2) {  // the smaller instantiations give the same bits (NaN = NaN here)
        double q2[2], pit2;
        int it2;
        sgp::mq_point<2>(mean.data() + s0 * T + t, var.data() + s0 * T + t, info.data() + s0, off[g + 1] - s0, T, Q, pr, has_y,
                         has_y ? y[g * T + t] : 0.0, q2, &pit2, &it2);
        for (int q = 0; q < Q; ++q)
          if (!(q2[q] == quant[q] || (q2[q] != q2[q] && quant[q] != quant[q]))) return 3;
        if (it2 != iters) return 3;
      }
      printf("%lld %lld %d %a", g, t, iters, pit);
      for (int q = 0; q < Q; ++q) printf(" %a", quant[q]);
      for (int q = 0; q < Q; ++q)
        printf(" %a", control(mean.data() + s0 * T + t, var.data() + s0 * T + t, info.data() + s0, off[g + 1] - s0, T, pr.p_tail[q],
                              pr.upper[q]));
      printf("\n");
    }
  }
  printf("mixture quantile host ok\n");
  return 0;
}
