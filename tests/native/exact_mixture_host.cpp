// Stand-alone host program: the per-point arithmetic of the mixture over draws (csrc/sgp_exact_predict.hpp: ep_mix_point) on cases read
// from a text file, results printed as hexadecimal floats.  Built by g++ alone (tests/test_exact_predict.py builds it with
// AddressSanitizer + UBSan); nothing of HIP is needed.
//
// Input:  G T P has_y / offsets[G + 1] / info[P] / mean[P x T] / var[P x T] / y[G x T] (has_y)
// Output: one line per (g, t):  g t kept mean var logpdf mean_logpdf
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sgp_exact_predict.hpp"

static bool read_doubles(FILE* f, std::vector<double>& v) {
  for (double& x : v) {
    char tok[64];
    if (fscanf(f, "%63s", tok) != 1) return false;
    x = strtod(tok, nullptr);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  long long G, T, P;
  int has_y;
  if (fscanf(f, "%lld %lld %lld %d", &G, &T, &P, &has_y) != 4 || G < 1 || T < 1 || P < 0) return 2;
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
  for (long long g = 0; g < G; ++g) {
    if (off[g + 1] < off[g]) return 2;
    for (long long t = 0; t < T; ++t) {
      const long long s0 = off[g];
      const sgp::EpMixPoint r = sgp::ep_mix_point(mean.data() + s0 * T + t, var.data() + s0 * T + t, info.data() + s0, off[g + 1] - s0, T,
                                                  has_y, has_y ? y[g * T + t] : 0.0);
      printf("%lld %lld %lld %a %a %a %a\n", g, t, (long long)r.kept, r.mean, r.var, r.logpdf, r.mean_logpdf);
    }
  }
  printf("exact mixture ok\n");
  return 0;
}
