// Stand-alone check of the likelihood layer csrc/sgp_lik.hpp on the host (built with AddressSanitizer + UBSan by tests/test_lik_host.py):
// every likelihood function on a grid of (y, mu, var) against the same 20-point Gauss-Hermite sum (or closed form) evaluated in long
// double, and its dmu / dv against central differences of that long-double sum in mu and in var.  The grid reaches y f = -60 under both
// Bernoulli links, y = 0 and y = 10^6 under Poisson, var at and below the floor of the SGPMC row pass, and mu + var / 2 > 709.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "sgp_lik.hpp"

using namespace sgp;
typedef long double ld;

static GHTable gh;
static int failures = 0, checks = 0;

static void expect(bool ok, const char* what, int lik, double y, double mu, double var, double got, ld want) {
  ++checks;
  if (ok) return;
  ++failures;
  if (failures <= 20) std::printf("FAIL %s lik %d y %g mu %g var %g: got %.17g want %.17Lg\n", what, lik, y, mu, var, got, want);
}

// the energy of one datum in long double, and the size of its terms (what a float64 evaluation can be held to)
// (a function of sd = sqrt(var), in which every one of them is even and smooth: the differences below are taken in sd)
static ld ell_ld(int lik, ld y, ld mu, ld sd, ld s2, ld* scale) {
  const ld PI = acosl(-1.0L);
  const ld var = sd * sd;
  if (lik == 0) {
    const ld r = y - mu, q = r * r + var;
    *scale = 1.0L + fabsl(logl(s2)) + q / (2 * s2);
    return -logl(2 * PI) / 2 - logl(s2) / 2 - q / (2 * s2);
  }
  if (lik == 3) {
    const ld E = expl(mu + var / 2), lg = lgammal(y + 1);
    *scale = fabsl(y * mu) + E + fabsl(lg) + 1.0L;
    return y * mu - E - lg;
  }
  ld s = 0, a = 0;
  for (int i = 0; i < GH_N; ++i) {
    const ld z = y * (mu + sd * (ld)gh.x[i]);
    ld lp;
    if (lik == 1) lp = z < 0 ? logl(erfcl(-z / sqrtl(2.0L)) / 2) : log1pl(-erfcl(z / sqrtl(2.0L)) / 2);
    else lp = z < 0 ? z - log1pl(expl(z)) : -log1pl(expl(-z));
    s += (ld)gh.w[i] * lp;
    a += (ld)gh.w[i] * fabsl(lp);
  }
  *scale = a + 1.0L;
  return s;
}

static void check_point(int lik, double y, double mu, double var, double s2) {
  double ell, gm, gv, gs;
  lik_eval(lik, y, mu, var, s2, gh, ell, gm, gv, gs);
  ld scale, sc2;
  const ld sd = sqrtl((ld)var);
  const ld want = ell_ld(lik, y, mu, sd, s2, &scale);
  expect(std::fabs((ld)ell - want) <= 1e-13L * scale, "ell", lik, y, mu, var, ell, want);
  // central differences in mu and in sd (d / d var = (d / d sd) / (2 sd); the sum is even in sd, so sd - h < 0 is no obstacle):
  // truncation h^2 f(3) / 6 is below 1e-7 of the sizes involved, the quotient's own rounding is 4 eps_ld scale / h
  const ld eps = std::numeric_limits<ld>::epsilon();
  const ld hm = 1e-5L * (1.0L + fabsl((ld)mu)), hd = 1e-4L;
  const ld dm = (ell_ld(lik, y, mu + hm, sd, s2, &sc2) - ell_ld(lik, y, mu - hm, sd, s2, &sc2)) / (2 * hm);
  const ld dvv = (ell_ld(lik, y, mu, sd + hd, s2, &sc2) - ell_ld(lik, y, mu, sd - hd, s2, &sc2)) / (2 * hd) / (2 * sd);
  expect(std::fabs((ld)gm - dm) <= 1e-7L * (fabsl(dm) + scale / (1.0L + fabsl((ld)mu))) + 4 * eps * scale / hm, "dmu", lik, y, mu, var, gm, dm);
  expect(std::fabs((ld)gv - dvv) <= 1e-7L * (fabsl(dvv) + fabsl(dm) + 1.0L) + 4 * eps * scale / (hd * 2 * sd), "dv", lik, y, mu, var, gv, dvv);
  if (lik == 0) {
    const ld hs = 1e-5L * (ld)s2;
    const ld ds = (ell_ld(0, y, mu, sd, s2 + hs, &sc2) - ell_ld(0, y, mu, sd, s2 - hs, &sc2)) / (2 * hs);
    expect(std::fabs((ld)gs - ds) <= 1e-7L * (fabsl(ds) + 1.0L), "ds2", lik, y, mu, var, gs, ds);
  } else {
    expect(gs == 0.0, "ds2 = 0", lik, y, mu, var, gs, 0);
  }
}

int main() {
  gh = make_gh();
  double sw = 0.0, sx2 = 0.0;
  for (int i = 0; i < GH_N; ++i) { sw += gh.w[i]; sx2 += gh.w[i] * gh.x[i] * gh.x[i]; }
  expect(std::fabs(sw - 1.0) < 1e-14 && std::fabs(sx2 - 1.0) < 1e-13, "Gauss-Hermite table", -1, 0, 0, 0, sw, 1);

  const double sf2 = 1.0, floor = sf2 * 0x1p-40;
  const double vars[] = {floor, 1e-9, 1e-6, 0.3, 2.5};
  // ---- the two Bernoulli links: y f from +40 down to -60 ----
  const double mus[] = {-60.0, -40.0, -5.0, 0.0, 0.7, 3.0, 40.0, 60.0};
  for (int lik = 1; lik <= 2; ++lik)
    for (double y : {-1.0, 1.0})
      for (double mu : mus)
        for (double var : vars) check_point(lik, y, mu, var, 1.0);
  // ---- Gaussian ----
  for (double y : {-2.0, 0.3})
    for (double mu : {-1.0, 0.0, 4.0})
      for (double var : vars)
        for (double s2 : {1e-3, 0.1, 7.0}) check_point(0, y, mu, var, s2);
  // ---- Poisson: y = 0 and y = 10^6 included ----
  for (double y : {0.0, 3.0, 1e6})
    for (double mu : {-3.0, 0.5, 5.0, 13.8})
      for (double var : vars) check_point(3, y, mu, var, 1.0);
  // ---- var at and below the floor: raised to it, dv = 0; the floor itself is not floored ----
  for (int lik = 0; lik <= 3; ++lik)
    for (double var : {floor, 0.5 * floor, 0.0, -1e-17}) {
      const double y = lik == 3 ? 2.0 : 1.0, mu = 0.4;
      double e0, m0, v0, s0, e1, m1, v1, s1;
      lik_eval(lik, y, mu, floor, 0.5, gh, e0, m0, v0, s0);
      lik_eval_floored(lik, y, mu, var, floor, 0.5, gh, e1, m1, v1, s1);
      expect(e1 == e0 && m1 == m0 && s1 == s0, "floored value", lik, y, mu, var, e1, e0);
      expect(var < floor ? v1 == 0.0 : v1 == v0, "floored dv", lik, y, mu, var, v1, var < floor ? 0.0 : v0);
    }
  {  // a NaN variance is not below the floor: it stays NaN
    double e, m, v, s;
    lik_eval_floored(3, 1.0, 0.0, std::numeric_limits<double>::quiet_NaN(), floor, 1.0, gh, e, m, v, s);
    expect(std::isnan(e) && std::isnan(v), "NaN variance", 3, 1, 0, 0, e, 0);
  }
  // ---- mu + var / 2 > 709: exp overflows to +inf, the energy is -inf, nothing else happens ----
  for (double y : {0.0, 5.0}) {
    double e, m, v, s;
    lik_eval(3, y, 708.0, 4.0, 1.0, gh, e, m, v, s);
    expect(std::isinf(e) && e < 0 && std::isinf(m) && m < 0 && std::isinf(v) && v < 0, "Poisson overflow", 3, y, 708, 4, e, -INFINITY);
    lik_eval(3, y, 700.0, 4.0, 1.0, gh, e, m, v, s);
    expect(std::isfinite(e) && std::isfinite(m) && std::isfinite(v), "Poisson below overflow", 3, y, 700, 4, e, 0);
  }
  // ---- both Bernoulli tails finite at |y f| = 300 (no overflow of exp(+z), no 0 / 0) ----
  for (int lik = 1; lik <= 2; ++lik)
    for (double mu : {-300.0, 300.0}) {
      double e, m, v, s;
      lik_eval(lik, 1.0, mu, 1.0, 1.0, gh, e, m, v, s);
      expect(std::isfinite(e) && std::isfinite(m) && std::isfinite(v) && e <= 0.0, "Bernoulli far tail", lik, 1, mu, 1, e, 0);
    }
  std::printf("%d checks, %d failures\n", checks, failures);
  if (failures == 0) std::printf("likelihood layer ok\n");
  return failures == 0 ? 0 : 1;
}
