// Stand-alone check of lik_robustmax_pv (csrc/sgp_lik.hpp: the robust-max likelihood with one variance PER CLASS) on the host: a grid of
// (C, y, mu, var) against the same 20-point Gauss-Hermite sum evaluated in long double, and gm / gv against central differences of that
// long-double sum.  C in {2, 3, 16}, |mu| up to 40, per-class variances from the floor (2^-40) to 100 -- all equal, independently drawn,
// and strongly unequal (one class a factor 1e6 away from the others) --, ties, saturated data, variances below the floor, labels that are
// no class (NaN, no index formed), the strided layout the device uses, and the identity with lik_robustmax at equal variances.  Its own
// main(): it may be built with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include "sgp_lik.hpp"

using namespace sgp;
typedef long double ld;

static GHTable gh;
static int failures = 0, checks = 0;
static const double FLOOR = 0x1p-40;

static void expect(bool ok, const char* what, int C, double y, int c, double got, ld want) {
  ++checks;
  if (ok) return;
  ++failures;
  if (failures <= 20) std::printf("FAIL %s C %d y %g class %d: got %.17g want %.17Lg\n", what, C, y, c, got, want);
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

// p in long double as a function of the means and the standard deviations, and sum_i w_i P_i sum_c |log Phi| (the size of the exponent's
// terms: exp() turns their rounding into a relative error of p)
static ld p_ld(int C, int y, const ld* mu, const ld* sd, ld* expo) {
  ld p = 0, e = 0;
  for (int i = 0; i < GH_N; ++i) {
    ld s = 0, a = 0;
    for (int c = 0; c < C; ++c) {
      if (c == y) continue;
      const ld lp = log_ndtr_ld((mu[y] + sd[y] * (ld)gh.x[i] - mu[c]) / sd[c]);
      s += lp;
      a += fabsl(lp);
    }
    p += (ld)gh.w[i] * expl(s);
    e += (ld)gh.w[i] * expl(s) * a;
  }
  *expo = e;
  return p;
}

// The condition scale of sum_i r_ic (r_ic = P_i phi / Phi): the sum itself plus what a relative rounding of every z_id does to it to first
// order, sum_i r_ic (1 + sum_d phi/Phi(z_id) a_id + |z_ic + phi/Phi(z_ic)| a_ic) with a_id = |a_d| + |b_d x_i| the size of z_id's two terms
// (the rule of tests/svgp_mc_reference.py).  Returns the sum over the classes c != y.
static ld cond_ld(int C, int y, const ld* mu, const ld* sd) {
  ld total = 0;
  const ld half_log_2pi = logl(2 * acosl(-1.0L)) / 2;
  for (int i = 0; i < GH_N; ++i) {
    ld s = 0, z[16], r[16], az[16], sra = 0;
    for (int c = 0; c < C; ++c) {
      if (c == y) continue;
      z[c] = (mu[y] + sd[y] * (ld)gh.x[i] - mu[c]) / sd[c];
      az[c] = fabsl(mu[y] - mu[c]) / sd[c] + fabsl(sd[y] * (ld)gh.x[i]) / sd[c];
      const ld lp = log_ndtr_ld(z[c]);
      r[c] = expl(-z[c] * z[c] / 2 - half_log_2pi - lp);
      s += lp;
      sra += r[c] * az[c];
    }
    const ld P = (ld)gh.w[i] * expl(s);
    for (int c = 0; c < C; ++c)
      if (c != y) total += P * r[c] * (1 + sra + fabsl(z[c] + r[c]) * az[c]);
  }
  return total;
}

static void check_point(int C, int y, const double* mu, const double* var, double eps) {
  double ell, gm[16], gv[16];
  lik_robustmax_pv(C, (double)y, mu, var, 1, FLOOR, eps, gh, ell, gm, gv);
  ld m[16], sd[16];
  ld sdmin = 1e300L;
  for (int c = 0; c < C; ++c) {
    m[c] = mu[c];
    sd[c] = sqrtl((ld)var[c]);
    if (c != y && sd[c] < sdmin) sdmin = sd[c];
  }
  const ld l1 = log1pl(-(ld)eps), l0 = logl((ld)eps / (C - 1)), kap = l1 - l0;
  ld expo;
  const ld p = p_ld(C, y, m, sd, &expo);
  const ld want = p * l1 + (1 - p) * l0;
  // float64: p to 1e-15 (1 + the exponent's terms)
  expect(std::fabs((ld)ell - want) <= 1e-14L * (fabsl(l0) + kap * (p + expo)), "ell", C, y, -1, ell, want);
  expect(std::isfinite(ell), "ell finite", C, y, -1, ell, want);
  // Central differences of the long-double sum, Richardson-extrapolated ((4 D(h / 2) - D(h)) / 3), in each mean and each standard
  // deviation (d / d var_c = (d / d sd_c) / (2 sd_c)).  Every derivative is compared in the unit of its own step, in which all 2 C of
  // them are sums of kappa P_i phi / Phi times factors of order z or x:
  //   mean c != y:  step 1e-6 sd_c    (moves z_c by 1e-6),              unit sd_c
  //   mean y:       step 1e-6 sd_min  (moves z_c by 1e-6 sd_min / sd_c), unit sd_min            (sd_min over the classes c != y)
  //   sd c != y:    step 1e-6 sd_c    (moves z_c by 1e-6 z_c),          unit v_c  for gv[c]
  //   sd y:         step 1e-6 sd_min  (moves z_c by 1e-6 x sd_min / sd_c), unit 2 sd_y sd_min for gv[y]
  // Bound: 1e-6 of the largest derivative of the datum in those units (truncation after Richardson: the fourth power of the relative
  // move of log P, and the float64 side, 1e-15 of the same sums with absolute values) + the rounding of the quotient: p(up) and p(down)
  // carry 2 eps_ld (p + expo) each, eps_ld = 1.08e-19, so D(h) = (up - down) / (2 h) carries 4 eps_ld / 2e-6 = 2.2e-13, D(h / 2) twice
  // that, and (4 D(h / 2) - D(h)) / 3 at most (4 x 4.4e-13 + 2.2e-13) / 3 = 6.5e-13, times kappa (p + expo): 7e-13 of it (a datum that
  // is all but saturated has derivatives of 1e-9 kappa and below: there this term is the whole bound).
  auto central = [&](int k, ld step) {  // k < C: mean k; k >= C: sd of class k - C
    ld up, dn, e2;
    ld* arr = k < C ? m : sd;
    const int c = k < C ? k : k - C;
    const ld keep = arr[c];
    arr[c] = keep + step; up = p_ld(C, y, m, sd, &e2);
    arr[c] = keep - step; dn = p_ld(C, y, m, sd, &e2);
    arr[c] = keep;
    return kap * (up - dn) / (2 * step);
  };
  ld dwant[32], got[32], gmax = 0;
  for (int k = 0; k < 2 * C; ++k) {
    const int c = k < C ? k : k - C;
    const ld h = 1e-6L * (c == y ? sdmin : sd[c]);
    const ld unit = c == y ? sdmin : sd[c];  // d / d(mean or sd), made dimensionless by the step's own size
    dwant[k] = (4 * central(k, h / 2) - central(k, h)) / 3 * unit;
    got[k] = k < C ? (ld)gm[c] * unit : (ld)gv[c] * 2 * sd[c] * unit;
    if (fabsl(dwant[k]) > gmax) gmax = fabsl(dwant[k]);
  }
  const ld bound = 1e-6L * gmax + 7e-13L * kap * (p + expo) + 1e-300L;
  for (int k = 0; k < 2 * C; ++k)
    expect(fabsl(got[k] - dwant[k]) <= bound, k < C ? "gm" : "gv", C, y, k < C ? k : k - C, (double)got[k], dwant[k]);
  ld sum = 0, gbig = 0;  // a common shift of the means changes nothing
  for (int c = 0; c < C; ++c) {
    sum += gm[c];
    gbig = fabsl((ld)gm[c]) > gbig ? fabsl((ld)gm[c]) : gbig;
  }
  expect(fabsl(sum) <= 1e-15L * (C + 2) * gbig + 1e-300L, "sum gm", C, y, -1, (double)sum, 0);  // (+ 1e-300: subnormal entries)
}

int main() {
  gh = make_gh();
  const double eps = 1e-3;
  unsigned long long state = 88172645463325252ULL;
  auto rnd = [&]() {  // xorshift: uniform in (-1, 1)
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
  };
  const double vars[] = {0x1p-40, 1e-6, 1e-2, 0.3, 1.0, 7.0, 100.0};
  for (int C : {2, 3, 16})
    for (int mode = 0; mode < 4; ++mode)      // 0: all variances equal, 1: drawn independently, 2 / 3: one class 1e6 below / above the others
      for (double base : vars)
        for (double amp : {0.0, 0.1, 1.0, 5.0, 40.0})
          for (int rep = 0; rep < 2; ++rep) {
            if (mode >= 2 && base < 1e-6) continue;  // base / 1e6 stays at or above the floor
            double mu[16], var[16];
            for (int c = 0; c < C; ++c) {
              mu[c] = amp * rnd();
              var[c] = mode == 1 ? vars[(int)((rnd() + 1.0) * 3.49)] : base;
            }
            const int odd = ((int)((rnd() + 1.0) * 8.0)) % C;
            if (mode == 2) var[odd] = base * 1e-6;
            if (mode == 3)
              for (int c = 0; c < C; ++c)
                if (c != odd) var[c] = base * 1e-6;
            for (int y : {0, C / 2, C - 1}) check_point(C, y, mu, var, eps);
          }
  // equal variances: gm is lik_robustmax's and sum_c gv[c] its gv, to a few ulp of the condition scale (cond_ld: b = sqrt(v) / sqrt(v) is 1
  // to an ulp only, which moves every z_ic by an ulp of x_i) -- kappa cond / sd for gm, and for sum gv the x terms that cancel inside it:
  // kappa cond (max_c |delta_c| + |x|_max) / (2 v), twice (the labelled class's entry holds them once more)
  for (int C : {2, 3, 16})
    for (double var : vars)
      for (double amp : {0.0, 0.1, 1.0, 5.0, 40.0})
        for (int y : {0, C - 1}) {
          double mu[16], vv[16], gm[16], gv[16], gm1[16], ell, ell1, gv1;
          for (int c = 0; c < C; ++c) {
            mu[c] = amp * rnd();
            vv[c] = var;
          }
          lik_robustmax_pv(C, (double)y, mu, vv, 1, FLOOR, eps, gh, ell, gm, gv);
          lik_robustmax(C, (double)y, mu, var, eps, gh, ell1, gm1, gv1);
          const double sd = std::sqrt(var), u = 2.3e-16;
          ld m[16], sdl[16];
          double sv = 0.0, dmax = 0.0;
          for (int c = 0; c < C; ++c) {
            m[c] = mu[c];
            sdl[c] = sqrtl((ld)var);
            sv += gv[c];
            dmax = std::fmax(dmax, std::fabs(mu[y] - mu[c]) / sd);
          }
          const double kap = std::log1p(-eps) - std::log(eps / (C - 1));
          const double scale_m = kap * (double)cond_ld(C, y, m, sdl) / sd + 1e-300, scale_v = scale_m * (dmax + 7.62) / sd;
          for (int c = 0; c < C; ++c) expect(std::fabs(gm[c] - gm1[c]) <= 8 * u * scale_m, "equal-variance gm", C, y, c, gm[c], gm1[c]);
          expect(std::fabs(sv - gv1) <= 8 * u * scale_v, "equal-variance sum gv", C, y, -1, sv, gv1);
        }
  // ties at equal variances: p = 1 / C to the quadrature's error, every off-label gm the same, sum_c gv[c] = 0 to rounding
  for (int C : {2, 3, 16}) {
    double mu[16], vv[16], gm[16], gv[16], ell;
    for (int c = 0; c < C; ++c) {
      mu[c] = 0.7;
      vv[c] = 2.0;
    }
    lik_robustmax_pv(C, 1.0, mu, vv, 1, FLOOR, eps, gh, ell, gm, gv);
    const ld p = ((ld)ell - logl((ld)eps / (C - 1))) / (log1pl(-(ld)eps) - logl((ld)eps / (C - 1)));
    ld m[16], sd[16], expo;
    for (int c = 0; c < C; ++c) {
      m[c] = mu[c];
      sd[c] = sqrtl(2.0L);
    }
    expect(fabsl(p - p_ld(C, 1, m, sd, &expo)) < 1e-14L, "tie p (rule)", C, 1, -1, (double)p, 1.0L / C);
    expect(fabsl(p - 1.0L / C) < 1e-3L / C, "tie p", C, 1, -1, (double)p, 1.0L / C);
    double sv = 0.0, sa = 0.0;
    for (int c = 0; c < C; ++c) {
      sv += gv[c];
      sa += std::fabs(gv[c]);
    }
    expect(std::fabs(sv) <= 16 * 2.3e-16 * sa, "tie sum gv", C, 1, -1, sv, 0);
    for (int c = 2; c < C; ++c) expect(gm[c] == gm[0] && gv[c] == gv[0], "tie gm / gv", C, 1, c, gm[c], gm[0]);
  }
  // saturated at variances BELOW the floor (0 and 2^-60: raised to 2^-40, gv = 0 exactly): the labelled class far ahead (p = 1) or far
  // behind (p = 0): zero gradient, finite ell
  for (int C : {2, 3, 16})
    for (int lead : {0, 1}) {
      double mu[16], vv[16], gm[16], gv[16], ell;
      for (int c = 0; c < C; ++c) {
        mu[c] = -40.0;
        vv[c] = (c & 1) ? 0.0 : 0x1p-60;
      }
      mu[lead] = 40.0;
      lik_robustmax_pv(C, 0.0, mu, vv, 1, FLOOR, eps, gh, ell, gm, gv);
      const double want = lead == 0 ? std::log1p(-eps) : std::log(eps / (C - 1));
      expect(std::fabs(ell - want) <= 20 * 2.3e-16 * std::fabs(std::log(eps / (C - 1))), "saturated ell", C, 0, lead, ell, want);
      for (int c = 0; c < C; ++c) expect(gm[c] == 0.0 && gv[c] == 0.0, "saturated gm / gv", C, 0, c, gm[c], 0);
    }
  // the floor: a variance below it gives the values AT the floor and gv = 0 for that class alone; a NaN variance is not below anything
  {
    double mu[3] = {0.3, -0.2, 0.1}, lo[3] = {0.5, 1e-15, 2.0}, at[3] = {0.5, FLOOR, 2.0}, gm[3], gv[3], gm2[3], gv2[3], ell, ell2;
    for (int y = 0; y < 3; ++y) {
      lik_robustmax_pv(3, (double)y, mu, lo, 1, FLOOR, eps, gh, ell, gm, gv);
      lik_robustmax_pv(3, (double)y, mu, at, 1, FLOOR, eps, gh, ell2, gm2, gv2);
      expect(ell == ell2 && gm[0] == gm2[0] && gm[1] == gm2[1] && gm[2] == gm2[2], "floor values", 3, y, -1, ell, ell2);
      expect(gv[1] == 0.0 && gv[0] == gv2[0] && gv[2] == gv2[2] && (y != 1 || gv2[1] != 0.0), "floor gv", 3, y, 1, gv[1], 0);
    }
    double nv[3] = {0.5, (double)NAN, 2.0};
    lik_robustmax_pv(3, 0.0, mu, nv, 1, FLOOR, eps, gh, ell, gm, gv);
    expect(std::isnan(ell) && std::isnan(gv[1]), "NaN variance stays NaN", 3, 0, 1, ell, 0);
  }
  // the device's layout: class c at [c * stride]; the same bits as the plain arrays, in place (gm = mu, gv = var) too
  {
    const int C = 5, S = 7;
    double mu[C], var[C], gm[C], gv[C], ell, ell2, smu[C * S], svar[C * S], sgm[C * S], sgv[C * S];
    for (int c = 0; c < C; ++c) {
      mu[c] = 2.0 * rnd();
      var[c] = 0.1 + (rnd() + 1.0);
    }
    for (int col = 0; col < S; ++col)
      for (int c = 0; c < C; ++c) {
        smu[c * S + col] = col == 3 ? mu[c] : 100.0 + col;
        svar[c * S + col] = col == 3 ? var[c] : 50.0;
        sgm[c * S + col] = sgv[c * S + col] = -7.0;
      }
    lik_robustmax_pv(C, 2.0, mu, var, 1, FLOOR, eps, gh, ell, gm, gv);
    lik_robustmax_pv(C, 2.0, smu + 3, svar + 3, S, FLOOR, eps, gh, ell2, sgm + 3, sgv + 3);
    bool same = ell == ell2, untouched = true;
    for (int col = 0; col < S; ++col)
      for (int c = 0; c < C; ++c) {
        if (col == 3) same = same && sgm[c * S + 3] == gm[c] && sgv[c * S + 3] == gv[c];
        else untouched = untouched && sgm[c * S + col] == -7.0 && sgv[c * S + col] == -7.0;
      }
    expect(same, "strided layout", C, 2, -1, ell2, ell);
    expect(untouched, "strided layout writes its own column only", C, 2, -1, 0, 0);
    lik_robustmax_pv(C, 2.0, smu + 3, svar + 3, S, FLOOR, eps, gh, ell2, smu + 3, svar + 3);
    same = ell == ell2;
    for (int c = 0; c < C; ++c) same = same && smu[c * S + 3] == gm[c] && svar[c * S + 3] == gv[c];
    expect(same, "in place", C, 2, -1, ell2, ell);
  }
  // labels that are no class: NaN everywhere, and no index is formed from them (the sanitizers watch the arrays)
  for (double y : {-1.0, 3.0, 0.5, 2.5, 1e300, -1e300, (double)NAN, (double)INFINITY}) {
    double mu[3] = {0.1, 0.2, 0.3}, vv[3] = {1.0, 2.0, 3.0}, gm[3] = {7.0, 7.0, 7.0}, gv[3] = {7.0, 7.0, 7.0}, ell = 0.0;
    lik_robustmax_pv(3, y, mu, vv, 1, FLOOR, eps, gh, ell, gm, gv);
    expect(std::isnan(ell) && std::isnan(gv[0]) && std::isnan(gv[2]) && std::isnan(gm[0]) && std::isnan(gm[2]), "bad label", 3, y, -1, ell, 0);
  }
  std::printf("robust-max per-class-variance layer ok: %d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
