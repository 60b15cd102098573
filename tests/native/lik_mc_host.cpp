// Stand-alone check of lik_robustmax (csrc/sgp_lik.hpp) on the host: a grid of (C, y, mu, var) against the same 20-point Gauss-Hermite
// sum evaluated in long double, and gm / gv against central differences of that long-double sum.  C in {2, 3, 16}, |mu| up to 40, var
// from the floor of the SGPMC row pass (2^-40) to 100, ties (all means equal: p = 1 / C to the quadrature's error, gv = 0 exactly),
// saturated data (p = 0 and p = 1: zero gradient, finite ell) and labels that are no class (NaN, no index formed).  Its own main():
// it may be built with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include "sgp_lik.hpp"

using namespace sgp;
typedef long double ld;

static GHTable gh;
static int failures = 0, checks = 0;

static void expect(bool ok, const char* what, int C, double y, double var, int c, double got, ld want) {
  ++checks;
  if (ok) return;
  ++failures;
  if (failures <= 20) std::printf("FAIL %s C %d y %g var %g class %d: got %.17g want %.17Lg\n", what, C, y, var, c, got, want);
}

static ld log_ndtr_ld(ld z) {
  const ld r2 = sqrtl(2.0L);
  if (z > 0) return log1pl(-erfcl(z / r2) / 2);
  if (z > -30.0L) return logl(erfcl(-z / r2) / 2);
  const ld t = -z / r2;  // erfc(t) = exp(-t^2) / (t sqrt pi) (1 - 1 / (2 t^2) + 3 / (4 t^4) - ...)
  ld s = 1.0L, term = 1.0L;
  for (int k = 1; k < 30; ++k) {
    term *= -(ld)(2 * k - 1) / (2 * t * t);
    s += term;
  }
  return -t * t - logl(t * sqrtl(acosl(-1.0L))) + logl(s) - logl(2.0L);
}

// p in long double as a function of the means and sd, and sum_i w_i P_i sum_c |log Phi| (the size of the exponent's terms)
static ld p_ld(int C, int y, const ld* mu, ld sd, ld* expo) {
  ld p = 0, e = 0;
  for (int i = 0; i < GH_N; ++i) {
    ld s = 0, a = 0;
    for (int c = 0; c < C; ++c) {
      if (c == y) continue;
      const ld lp = log_ndtr_ld((ld)gh.x[i] + (mu[y] - mu[c]) / sd);
      s += lp;
      a += fabsl(lp);
    }
    p += (ld)gh.w[i] * expl(s);
    e += (ld)gh.w[i] * expl(s) * a;
  }
  *expo = e;
  return p;
}

static void check_point(int C, int y, const double* mu, double var, double eps) {
  double ell, gv, gm[16];
  lik_robustmax(C, (double)y, mu, var, eps, gh, ell, gm, gv);
  ld m[16];
  for (int c = 0; c < C; ++c) m[c] = mu[c];
  const ld sd = sqrtl((ld)var);
  const ld l1 = log1pl(-(ld)eps), l0 = logl((ld)eps / (C - 1)), kap = l1 - l0;
  ld expo;
  const ld p = p_ld(C, y, m, sd, &expo);
  const ld want = p * l1 + (1 - p) * l0;
  // float64: p to 1e-15 (1 + the exponent's terms: exp() turns their rounding into a relative error of p)
  expect(std::fabs((ld)ell - want) <= 1e-14L * (fabsl(l0) + kap * (p + expo)), "ell", C, y, var, -1, ell, want);
  expect(std::isfinite(ell), "ell finite", C, y, var, -1, ell, want);
  // central differences of the long-double sum in each mean and in sd (d / d var = (d / d sd) / (2 sd)); step h relative to sd.
  // Bound: 1e-6 of the gradient's own size + of the largest one of the datum (truncation and the rounding 4 eps_ld / h of the quotient, see below), + 1e-13 of kappa p / sd for the float64 side.
  const ld h = 1e-6L * sd;
  ld gmax = 0, dwant[17];
  // (h = 1e-6 sd moves every z by 1e-6 |delta| and log p by z times that, up to 1e-3 in the far tails, where p ~ exp(-|z|^2 / 2) with
  // |z| ~ 36 over all classes; Richardson, (4 D(h / 2) - D(h)) / 3, removes the square of that and leaves its fourth power, 1e-12)
  auto central = [&](int c, ld step) {
    ld up, dn, e2;
    if (c < C) {
      const ld keep = m[c];
      m[c] = keep + step; up = p_ld(C, y, m, sd, &e2);
      m[c] = keep - step; dn = p_ld(C, y, m, sd, &e2);
      m[c] = keep;
      return kap * (up - dn) / (2 * step);
    }
    up = p_ld(C, y, m, sd + step, &e2);
    dn = p_ld(C, y, m, sd - step, &e2);
    return kap * (up - dn) / (2 * step) / (2 * sd);
  };
  for (int c = 0; c <= C; ++c) {
    dwant[c] = (4 * central(c, h / 2) - central(c, h)) / 3;
    if (fabsl(dwant[c]) > gmax) gmax = fabsl(dwant[c]);
  }
  const ld gscale = gmax + kap * (p + expo) / sd * 1e-7L + 1e-300L;
  for (int c = 0; c < C; ++c) expect(std::fabs((ld)gm[c] - dwant[c]) <= 1e-6L * gscale, "gm", C, y, var, c, gm[c], dwant[c]);
  expect(std::fabs((ld)gv - dwant[C]) <= 1e-6L * (gscale / sd + fabsl(dwant[C])), "gv", C, y, var, C, gv, dwant[C]);
  ld sum = 0;
  for (int c = 0; c < C; ++c) sum += gm[c];
  ld gbig = 0;  // (the code's own largest entry: where p = 1 to the last bit the differences above are 0)
  for (int c = 0; c < C; ++c) gbig = fabsl((ld)gm[c]) > gbig ? fabsl((ld)gm[c]) : gbig;
  expect(fabsl(sum) <= 1e-15L * (C + 2) * gbig, "sum gm", C, y, var, -1, (double)sum, 0);
}

int main() {
  gh = make_gh();
  const double eps = 1e-3;
  unsigned long long state = 88172645463325252ULL;
  auto rnd = [&]() {  // xorshift: uniform in (-1, 1)
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
  };
  for (int C : {2, 3, 16})
    for (double var : {0x1p-40, 1e-6, 1e-2, 0.3, 1.0, 7.0, 100.0})
      for (double amp : {0.0, 0.1, 1.0, 5.0, 40.0})
        for (int rep = 0; rep < 3; ++rep) {
          double mu[16];
          for (int c = 0; c < C; ++c) mu[c] = amp * rnd();
          for (int y : {0, C / 2, C - 1}) check_point(C, y, mu, var, eps);
        }
  // ties: p = 1 / C (to the quadrature's error on Phi^(C-1)), gv = 0 exactly, every off-label gm the same
  for (int C : {2, 3, 16}) {
    double mu[16], gm[16], ell, gv;
    for (int c = 0; c < C; ++c) mu[c] = 0.7;
    lik_robustmax(C, 1.0, mu, 2.0, eps, gh, ell, gm, gv);
    // p is the 20-point rule's value of  int Phi^(C-1) phi = 1 / C: the same sum in long double to rounding, 1 / C to the rule's own
    // error on Phi^(C-1), which is no polynomial (below 1e-3 of 1 / C up to C = 16)
    const ld p = ((ld)ell - logl((ld)eps / (C - 1))) / (log1pl(-(ld)eps) - logl((ld)eps / (C - 1)));
    ld m[16], expo;
    for (int c = 0; c < C; ++c) m[c] = mu[c];
    expect(fabsl(p - p_ld(C, 1, m, sqrtl(2.0L), &expo)) < 1e-14L, "tie p (rule)", C, 1, 2.0, -1, (double)p, 1.0L / C);
    expect(fabsl(p - 1.0L / C) < 1e-3L / C, "tie p", C, 1, 2.0, -1, (double)p, 1.0L / C);
    expect(gv == 0.0, "tie gv", C, 1, 2.0, -1, gv, 0);
    for (int c = 2; c < C; ++c) expect(gm[c] == gm[0], "tie gm", C, 1, 2.0, c, gm[c], gm[0]);
  }
  // saturated: the labelled class far ahead (p = 1) or far behind (p = 0), at the floor variance: zero gradient, finite ell
  for (int C : {2, 3, 16})
    for (int lead : {0, 1}) {
      double mu[16], gm[16], ell, gv;
      for (int c = 0; c < C; ++c) mu[c] = -40.0;
      mu[lead] = 40.0;
      lik_robustmax(C, 0.0, mu, 0x1p-40, eps, gh, ell, gm, gv);
      const double want = lead == 0 ? std::log1p(-eps) : std::log(eps / (C - 1));
      // (p is the sum of the 20 weights or 0: 1 to 20 roundings, which kappa ~ |log(eps / (C - 1))| carries into ell)
      expect(std::fabs(ell - want) <= 20 * 2.3e-16 * std::fabs(std::log(eps / (C - 1))), "saturated ell", C, 0, 0x1p-40, lead, ell, want);
      expect(gv == 0.0, "saturated gv", C, 0, 0x1p-40, lead, gv, 0);
      for (int c = 0; c < C; ++c) expect(gm[c] == 0.0, "saturated gm", C, 0, 0x1p-40, c, gm[c], 0);
    }
  // labels that are no class: NaN everywhere, and no index is formed from them (the sanitizers watch gm / mu)
  for (double y : {-1.0, 3.0, 0.5, 1e300, -1e300, (double)NAN, (double)INFINITY}) {
    double mu[3] = {0.1, 0.2, 0.3}, gm[3] = {7.0, 7.0, 7.0}, ell = 0.0, gv = 0.0;
    lik_robustmax(3, y, mu, 1.0, eps, gh, ell, gm, gv);
    expect(std::isnan(ell) && std::isnan(gv) && std::isnan(gm[0]) && std::isnan(gm[2]), "bad label", 3, y, 1.0, -1, ell, 0);
  }
  std::printf("robust-max layer ok: %d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
