// The likelihood layer: E_{N(mu, var)} log p(y | f) and its derivatives, one function per likelihood id of include/sgp.h.
// Shared by the SVGP minibatch bound (sgp_svgp.hip) and the SGPMC row pass (sgp_sgpmc_lik.hip); plain C++ apart from the
// __host__ __device__ markers, so a host compiler alone builds it (tests/native/lik_host.cpp).
//
//   (ell, dmu, dv, ds2) from (y, mu, var):   ell = E log p(y | f),  dmu = d ell / d mu,  dv = d ell / d var,  ds2 = d ell / d s2
//
// For the two Bernoulli links ell is the 20-point Gauss-Hermite sum  sum_i w_i log p(y | mu + sqrt(var) x_i), and dmu, dv are the
// derivatives OF THAT SUM, sum_i w_i (.)' and sum_i w_i x_i (.)' / (2 sqrt var) -- not the second-derivative form of Price's theorem,
// which differs from them by the quadrature error: a sampler needs the force to be the gradient of the energy it evaluates.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SGP_LIK_HD __host__ __device__ __forceinline__
#else
#define SGP_LIK_HD inline
#endif

namespace sgp {

constexpr int GH_N = 20;
struct GHTable {
  double x[GH_N];  // nodes of  int f(x) N(x; 0, 1) dx
  double w[GH_N];  // weights (sum to 1)
};
// Gauss-Hermite nodes / weights by Newton iteration on the orthonormal Hermite recurrence (host, once):
// physicists' rule (weight exp(-x^2)) rescaled to the standard normal:  x * sqrt(2),  w / sqrt(pi).
inline void gauss_hermite_host(int n, double* xs, double* ws) {
  const double PIM4 = 0.7511255444649425;  // pi^(-1/4)
  double z = 0.0, pp = 1.0;
  const int half = (n + 1) / 2;
  for (int i = 0; i < half; ++i) {
    if (i == 0) z = sqrt(2.0 * n + 1.0) - 1.85575 * pow(2.0 * n + 1.0, -0.16667);
    else if (i == 1) z -= 1.14 * pow((double)n, 0.426) / z;
    else if (i == 2) z = 1.86 * z - 0.86 * xs[0];
    else if (i == 3) z = 1.91 * z - 0.91 * xs[1];
    else z = 2.0 * z - xs[i - 2];
    for (int its = 0; its < 200; ++its) {
      double p1 = PIM4, p2 = 0.0;
      for (int j = 1; j <= n; ++j) {
        const double p3 = p2;
        p2 = p1;
        p1 = z * sqrt(2.0 / j) * p2 - sqrt((double)(j - 1) / j) * p3;
      }
      pp = sqrt(2.0 * n) * p2;
      const double z1 = z;
      z = z1 - p1 / pp;
      if (fabs(z - z1) <= 1e-15 * (1.0 + fabs(z))) break;
    }
    xs[i] = z;
    xs[n - 1 - i] = -z;
    ws[i] = ws[n - 1 - i] = 2.0 / (pp * pp);
  }
  for (int i = 0; i < n; ++i) {
    xs[i] *= 1.4142135623730951;
    ws[i] *= 0.5641895835477563;
  }
}
inline GHTable make_gh() {
  GHTable t;
  gauss_hermite_host(GH_N, t.x, t.w);
  return t;
}

// erfcx(t) = exp(t^2) erfc(t).  The device library has it; a host build (the stand-alone check of this header) forms it in long
// double, with the asymptotic series where erfc underflows.
SGP_LIK_HD double lik_erfcx(double t) {
#if defined(__HIP_DEVICE_COMPILE__)
  return erfcx(t);
#else
  const long double x = t;
  if (x < 25.0L) return (double)(expl(x * x) * erfcl(x));
  long double s = 1.0L, term = 1.0L;
  const long double x2 = 2.0L * x * x;
  for (int k = 1; k < 40; ++k) {
    term *= -(long double)(2 * k - 1) / x2;
    s += term;
    if (fabsl(term) < 1e-22L) break;
  }
  return (double)(s / (x * 1.7724538509055160272981674833411L));
#endif
}

// log Phi(z).  erfc underflows to 0 for z <= -38.6 (one mislabelled point against a confident mean reaches that at the outer
// Gauss-Hermite node, 7.62, and the whole minibatch bound became -inf): for z < 0 the scaled complementary error function,
// erfc(t) = erfcx(t) exp(-t^2), keeps the logarithm finite down to where z^2 / 2 itself overflows.
SGP_LIK_HD double log_ndtr_dev(double z) {
  if (z < 0.0) return log(0.5 * lik_erfcx(-z * 0.7071067811865476)) - 0.5 * z * z;
  return log(0.5 * erfc(-z * 0.7071067811865476));
}
// phi(z) / Phi(z); for z < 0 it is sqrt(2 / pi) / erfcx(-z / sqrt 2), free of the 0 / 0 of the two underflowing factors
SGP_LIK_HD double mills_dev(double z) {
  if (z < 0.0) return 0.7978845608028654 / lik_erfcx(-z * 0.7071067811865476);
  return 0.3989422804014327 * exp(-0.5 * z * z) / (0.5 * erfc(-z * 0.7071067811865476));
}

// SGP_LIK_GAUSSIAN: log N(y | f, s2), closed form
SGP_LIK_HD void lik_gaussian(double yb, double m, double vv, double s2, double& ell, double& gm, double& gv, double& gs) {
  const double r = yb - m, q = r * r + vv;
  ell = -0.9189385332046727 - 0.5 * log(s2) - q / (2.0 * s2);
  gm = r / s2;
  gv = -0.5 / s2;
  gs = -0.5 / s2 + q / (2.0 * s2 * s2);
}

// SGP_LIK_BERNOULLI_PROBIT: log Phi(y f), y in {-1, +1}
SGP_LIK_HD void lik_bernoulli_probit(double yb, double m, double vv, const GHTable& gh, double& ell, double& gm, double& gv) {
  const double sd = sqrt(vv);
  ell = 0.0; gm = 0.0; gv = 0.0;
  for (int i = 0; i < GH_N; ++i) {
    const double z = yb * (m + sd * gh.x[i]);
    ell = fma(gh.w[i], log_ndtr_dev(z), ell);
    const double r = gh.w[i] * yb * mills_dev(z);
    gm += r;
    gv = fma(r, gh.x[i], gv);
  }
  gv = gv / (2.0 * sd);
}

// SGP_LIK_BERNOULLI_LOGIT: log sigmoid(y f) = -softplus(-y f), y in {-1, +1}.  Both tails through exp(-|z|): nothing overflows.
//   z >= 0: -log1p(e^-z), derivative e^-z / (1 + e^-z);   z < 0: z - log1p(e^z), derivative 1 / (1 + e^z)
SGP_LIK_HD void lik_bernoulli_logit(double yb, double m, double vv, const GHTable& gh, double& ell, double& gm, double& gv) {
  const double sd = sqrt(vv);
  ell = 0.0; gm = 0.0; gv = 0.0;
  for (int i = 0; i < GH_N; ++i) {
    const double z = yb * (m + sd * gh.x[i]);
    const double e = exp(-fabs(z));
    const double l1p = log1p(e);
    const double ls = z < 0.0 ? z - l1p : -l1p;         // log sigmoid(z); a NaN z stays NaN through l1p
    const double sg = (z < 0.0 ? 1.0 : e) / (1.0 + e);  // sigmoid(-z)
    ell = fma(gh.w[i], ls, ell);
    const double r = gh.w[i] * yb * sg;
    gm += r;
    gv = fma(r, gh.x[i], gv);
  }
  gv = gv / (2.0 * sd);
}

// SGP_LIK_POISSON_LOG: y ~ Poisson(exp f), closed form  y mu - exp(mu + var / 2) - lgamma(y + 1).  exp() may overflow: ell = -inf then.
SGP_LIK_HD void lik_poisson_log(double yb, double m, double vv, double& ell, double& gm, double& gv) {
  const double E = exp(m + 0.5 * vv);
  ell = yb * m - E - lgamma(yb + 1.0);
  gm = yb - E;
  gv = -0.5 * E;
}

// SGP_LIK_MULTICLASS_ROBUSTMAX: C latent functions with means mu[0 .. C-1] and ONE shared variance vv, label yb in {0 .. C-1} (a double).
//   p   = sum_i w_i prod_{c != y} Phi(x_i + (mu_y - mu_c) / sqrt vv)         (the probability that the labelled function is the largest)
//   ell = p log(1 - eps) + (1 - p) log(eps / (C - 1))
// The product is exp(sum log Phi): a saturated node underflows to 0, never to NaN.  gm[c] = d ell / d mu_c and gv = d ell / d vv are the
// derivatives OF THAT SUM (the convention above).  gv has BOTH signs: negative where the labelled function leads, positive where it
// trails -- a datum the model gets wrong wants more variance.  A label that is no integer of 0 .. C-1 gives NaN everywhere and is never
// used as an index.  mu and gm must not overlap.
SGP_LIK_HD void lik_robustmax(int C, double yb, const double* mu, double vv, double eps, const GHTable& gh, double& ell, double* gm,
                              double& gv) {
  int yi = -1;
  if (yb >= 0.0 && yb < (double)C) {
    yi = (int)yb;
    if ((double)yi != yb) yi = -1;
  }
  if (yi < 0) {
    const double bad = NAN;
    ell = bad; gv = bad;
    for (int c = 0; c < C; ++c) gm[c] = bad;
    return;
  }
  const double isd = 1.0 / sqrt(vv), my = mu[yi];
  for (int c = 0; c < C; ++c) gm[c] = 0.0;
  double p = 0.0;
  for (int i = 0; i < GH_N; ++i) {
    double s = 0.0;
    for (int c = 0; c < C; ++c)
      if (c != yi) s += log_ndtr_dev(fma(my - mu[c], isd, gh.x[i]));
    const double P = gh.w[i] * exp(s);
    p += P;
    for (int c = 0; c < C; ++c)
      if (c != yi) gm[c] = fma(P, mills_dev(fma(my - mu[c], isd, gh.x[i])), gm[c]);  // d p / d delta_c so far, delta_c = (mu_y - mu_c) / sd
  }
  const double l1 = log1p(-eps), l0 = log(eps / (double)(C - 1)), kap = l1 - l0;
  ell = p * l1 + (1.0 - p) * l0;
  double sr = 0.0, srd = 0.0;
  for (int c = 0; c < C; ++c) {
    if (c == yi) continue;
    const double r = gm[c];
    sr += r;
    srd = fma(r, (my - mu[c]) * isd, srd);
    gm[c] = -kap * r * isd;
  }
  gm[yi] = kap * sr * isd;
  gv = -0.5 * kap * srd * (isd * isd);
}

constexpr int LIK_ID_MAX = 3;  // SGP_LIK_POISSON_LOG (SGP_LIK_MULTICLASS_ROBUSTMAX has entry points of its own: sgp_sgpmc_mc.hip)

// the likelihood `lik` (0..LIK_ID_MAX; the entry points check the range) at one datum
SGP_LIK_HD void lik_eval(int lik, double yb, double m, double vv, double s2, const GHTable& gh, double& ell, double& gm, double& gv,
                         double& gs) {
  gs = 0.0;
  if (lik == 0) lik_gaussian(yb, m, vv, s2, ell, gm, gv, gs);
  else if (lik == 1) lik_bernoulli_probit(yb, m, vv, gh, ell, gm, gv);
  else if (lik == 2) lik_bernoulli_logit(yb, m, vv, gh, ell, gm, gv);
  else lik_poisson_log(yb, m, vv, ell, gm, gv);
}

// ... with the conditional variance of the SGPMC row pass: var = k_nn - |a_n|^2 cancels to rounding at a datum that coincides with an
// inducing input, so a variance below `var_floor` (the row pass: 2^-40 sf2) is raised to it and its dv is 0 -- the floor does not move
// with the parameters.  A NaN variance is not below anything: it stays NaN.
SGP_LIK_HD void lik_eval_floored(int lik, double yb, double m, double vv, double var_floor, double s2, const GHTable& gh, double& ell,
                                 double& gm, double& gv, double& gs) {
  const bool floored = vv < var_floor;
  lik_eval(lik, yb, m, floored ? var_floor : vv, s2, gh, ell, gm, gv, gs);
  if (floored) gv = 0.0;
}

// SGP_LIK_MULTICLASS_ROBUSTMAX with one variance PER CLASS (the multi-class SVGP bound, sgp_svgp_mc.hip: every class has a q(u_c) of
// its own).  Class c's mean and variance are mu[c * stride], var[c * stride] (stride 1: plain arrays; the device keeps them class-major,
// stride = the padded minibatch).  With z_ic = (mu_y + sqrt(v_y) x_i - mu_c) / sqrt(v_c) = a_c + b_c x_i:
//   P[i] = w_i prod_{c != y} Phi(z_ic),  returned: p = sum_i P[i]   (the probability that function y is the largest)
// A variance below var_floor is raised to it (lik_eval_floored's rule).  yi must be a class index.
SGP_LIK_HD double robustmax_pv_nodes(int C, int yi, const double* mu, const double* var, long stride, double var_floor,
                                     const GHTable& gh, double* P /* GH_N */) {
  const double vy = var[yi * stride] < var_floor ? var_floor : var[yi * stride];
  const double sdy = sqrt(vy), my = mu[yi * stride];
  for (int i = 0; i < GH_N; ++i) P[i] = 0.0;
  for (int c = 0; c < C; ++c) {
    if (c == yi) continue;
    const double vc = var[c * stride] < var_floor ? var_floor : var[c * stride];
    const double isd = 1.0 / sqrt(vc), a = (my - mu[c * stride]) * isd, b = sdy * isd;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < GH_N; ++i) P[i] += log_ndtr_dev(fma(b, gh.x[i], a));
  }
  double p = 0.0;
  for (int i = 0; i < GH_N; ++i) {
    P[i] = gh.w[i] * exp(P[i]);
    p += P[i];
  }
  return p;
}

//   ell = p log(1 - eps) + (1 - p) log(eps / (C - 1)),  kappa = log(1 - eps) - log(eps / (C - 1)),  r_ic = P_i phi(z_ic) / Phi(z_ic),
//   R_c = sum_i r_ic,  X_c = sum_i r_ic x_i:
//   gm[c] = -kappa R_c / sqrt(v_c)                       gm[y] = kappa sum_c R_c / sqrt(v_c)
//   gv[c] = -kappa (a_c R_c + b_c X_c) / (2 v_c)         gv[y] = kappa sum_c X_c / (2 sqrt(v_y) sqrt(v_c))
// -- the derivatives OF THAT SUM, as above; with all variances equal gm is lik_robustmax's and sum_c gv[c] its gv.  The gv of a floored
// variance is 0.  A label that is no integer of 0 .. C-1 gives NaN everywhere and is never used as an index.  gm / gv use the same stride;
// gm may be mu and gv may be var (class c's inputs are read before its outputs are written, class y's before any).
SGP_LIK_HD void lik_robustmax_pv(int C, double yb, const double* mu, const double* var, long stride, double var_floor, double eps,
                                 const GHTable& gh, double& ell, double* gm, double* gv) {
  int yi = -1;
  if (yb >= 0.0 && yb < (double)C) {
    yi = (int)yb;
    if ((double)yi != yb) yi = -1;
  }
  if (yi < 0) {
    const double bad = NAN;
    ell = bad;
    for (int c = 0; c < C; ++c) gm[c * stride] = gv[c * stride] = bad;
    return;
  }
  const bool floored_y = var[yi * stride] < var_floor;
  const double vy = floored_y ? var_floor : var[yi * stride];
  const double sdy = sqrt(vy), my = mu[yi * stride];
  double P[GH_N];
  const double p = robustmax_pv_nodes(C, yi, mu, var, stride, var_floor, gh, P);
  const double l1 = log1p(-eps), l0 = log(eps / (double)(C - 1)), kap = l1 - l0;
  ell = p * l1 + (1.0 - p) * l0;
  double sr = 0.0, sx = 0.0;
  for (int c = 0; c < C; ++c) {
    if (c == yi) continue;
    const bool floored = var[c * stride] < var_floor;
    const double vc = floored ? var_floor : var[c * stride];
    const double isd = 1.0 / sqrt(vc), a = (my - mu[c * stride]) * isd, b = sdy * isd;
    double R = 0.0, X = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < GH_N; ++i) {
      const double r = P[i] * mills_dev(fma(b, gh.x[i], a));
      R += r;
      X = fma(r, gh.x[i], X);
    }
    gm[c * stride] = -kap * R * isd;
    gv[c * stride] = floored ? 0.0 : -0.5 * kap * fma(a, R, b * X) * (isd * isd);
    sr = fma(R, isd, sr);
    sx = fma(X, isd, sx);
  }
  gm[yi * stride] = kap * sr;
  gv[yi * stride] = floored_y ? 0.0 : 0.5 * kap * sx / sdy;
}

}  // namespace sgp
