// Quantiles and the probability integral transform (PIT) of an equal-weight mixture of Gaussians (sgp_mixture.hip): what one (group,
// test point) computes over the draws of its group, as plain C++ that a host program can run (tests/native/mixture_quantile_host.cpp),
// and the limits of the entry point.  This header includes nothing of HIP.  The contract (W, the iteration cap, the rounding bound) is
// stated in include/sgp_mixture.h; DESIGN 6e-9 has the derivations.
//
// The kept draws of a group (info == 0; n of them, in index order) give, with sigma_s = sqrt(v_s) and u_s = (x - mu_s) / (sigma_s sqrt 2),
//   lower tail  G-(x) = (1/n) sum_s erfc(-u_s) / 2 ;  upper tail  G+(x) = (1/n) sum_s erfc(+u_s) / 2 ;
//   density     g(x)  = (1/n) sum_s exp(-u_s^2) / (sigma_s sqrt(2 pi)).
// Every term of a tail is non-negative, so a tail keeps its relative accuracy however small it is.  The quantile at p is the root of
// G-(x) = p for p <= 1/2 and of G+(x) = 1 - p above; the caller passes p_tail = min(p, 1 - p) and the side.
//
// Passes.  A pass walks the draws once, serially, in index order, every sum from zero, and loads a draw's (mu, v) once for ALL the
// probabilities of the call:
//   pass 0    n, the smallest sigma, the bracket ends lo_q = min_s (mu_s - z_q sigma_s), hi_q = max_s (mu_s + z_q sigma_s) with z_q =
//             sqrt(-2 ln p_tail_q), and, with a target y, the PIT sum.  Phi(-z) <= exp(-z^2 / 2) / 2 = p_tail / 2: every component's
//             own quantile lies in [mu_s - z sigma_s, mu_s + z sigma_s], and the mixture's lies between the smallest and the largest
//             of them (at the smallest every component's CDF is <= p, at the largest >= p).
//   pass k    the tail and the density of every unfinished probability q at its current point x_q.
// A probability goes through: verify lo (its tail must be on the "quantile is above" side; else step outwards, doubling), verify hi,
// then iterate, from the point where the line through the two ends' log-tails meets log p_tail.  An iteration puts x into the bracket [a, b] (a: "above" side, b: the other), ends when b - a <= W(mid), and otherwise
// proposes a Newton step on the LOGARITHM of the tail (log-tails of Gaussians are close to parabolas: the plain tail is not, at
// p = 1e-9) pushed W / 4 past its target, so that a converged sequence lands on the other side of the root and closes the bracket;
// every time x lands on the side it came from, the push doubles (where the tail's rounding noise is wider than W -- a wide component
// beside a narrow sigma_min -- the other side is found in a logarithmic number of passes).  A proposal is taken only strictly inside
// (a, b), and after MQ_STALL proposals in a row that did not halve the bracket the next pass is a bisection (the proposal waits and is
// taken up after it); a zero density in the gap of a bimodal mixture, a tail equal to p_tail, a NaN are bisections too.  x never
// leaves the bracket and the bracket halves at least every MQ_STALL + 1 passes: the loop ends.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SGP_MQ_HD __host__ __device__
#define SGP_MQ_UNROLL _Pragma("unroll")  // the per-probability loops: their state stays in registers
#else
#define SGP_MQ_HD
#define SGP_MQ_UNROLL
#endif

namespace sgp {

constexpr int MQ_MAXQ = 8;                  // probabilities per call
constexpr double MQ_PMIN = 1e-9;            // MQ_PMIN <= p <= 1 - MQ_PMIN
constexpr int MQ_MAX_ITERS = 256;           // passes after pass 0 that one point may take; a probability not finished by then is NaN
constexpr int MQ_STALL = 3;                 // proposals in a row that may fail to halve the bracket before a bisection is forced
constexpr double MQ_WIDTH = 0x1p-48;        // W(x) = MQ_WIDTH (|x| + sigma_min): the final bracket's width
constexpr double MQ_ERFC_ULP = 2.9902;      // the device erfc's worst error in ulps (profiles/mixture_quantile_erfc_ulp.json)
constexpr double MQ_C = 2.0 * MQ_ERFC_ULP + 4.0;  // MQ_ERR(n, tail, sens) = 2^-52 ((n + MQ_C) tail + 2 sens)
constexpr int64_t MQ_MAXG = (1 << 24) - 1;  // groups (EB_MAXP)
constexpr int64_t MQ_MAXT = 32768;          // test points (EP_MAXT)

struct MqProbs {  // travels in the launch arguments
  double p_tail[MQ_MAXQ];
  int upper[MQ_MAXQ];
};

// SGP_OK = 0, SGP_ERR_ARG = -1: the probabilities a call accepts (a NaN fails both comparisons)
SGP_MQ_HD inline bool mq_prob_ok(double p) { return p >= MQ_PMIN && p <= 1.0 - MQ_PMIN; }

// p -> (p_tail, side); 1 - p is formed once, here, on the host
inline void mq_split(double p, double* p_tail, int* upper) {
  *upper = p > 0.5 ? 1 : 0;
  *p_tail = p > 0.5 ? 1.0 - p : p;
}

SGP_MQ_HD inline double mq_width(double x, double sigma_min) { return MQ_WIDTH * (fabs(x) + sigma_min); }

// One (group, test point): the draws are entries 0, stride, 2 stride, ... (n_draws of them) of mean / var, with info[s] per draw; a
// draw with info != 0 is skipped.  quant[q], q < Q <= NQ: the quantile at (pr.p_tail[q], pr.upper[q]); *pit (has_y): G-(y); *iters:
// the passes after pass 0 (the largest count over the probabilities).  n = 0, or a kept draw whose v is not positive and finite or
// whose mu is not finite: every output is NaN (iters 0).  NQ is the compile-time size of the per-probability state (registers on the
// device); the arithmetic of a probability does not depend on it, on Q, or on the other probabilities.
template <int NQ>
SGP_MQ_HD inline void mq_point(const double* mean, const double* var, const int* info, int64_t n_draws, int64_t stride, int Q,
                               const MqProbs& pr, int has_y, double y, double* quant, double* pit, int* iters) {
  const double nan = NAN, inf = INFINITY;
  const double rsqrt2 = 0.70710678118654752440, rsqrtpi = 0.56418958354775628695;
  double zq[NQ], lo[NQ], hi[NQ];
SGP_MQ_UNROLL
  for (int q = 0; q < NQ; ++q) {
    zq[q] = q < Q ? sqrt(-2.0 * log(pr.p_tail[q])) : 0.0;
    lo[q] = inf, hi[q] = -inf;
    if (q < Q) quant[q] = nan;
  }
  *pit = nan;
  *iters = 0;
  int64_t n = 0;
  bool bad = false;
  double smin = inf, spit = 0.0;
  for (int64_t s = 0; s < n_draws; ++s) {  // pass 0
    if (info[s] != 0) continue;
    ++n;
    const double mu = mean[s * stride], v = var[s * stride];
    if (!(v > 0.0) || !(v < inf) || !(fabs(mu) < inf)) {  // (a NaN fails every comparison)
      bad = true;
      continue;
    }
    const double sg = sqrt(v);
    smin = sg < smin ? sg : smin;
SGP_MQ_UNROLL
    for (int q = 0; q < NQ; ++q) {
      const double l = mu - zq[q] * sg, h = mu + zq[q] * sg;
      lo[q] = l < lo[q] ? l : lo[q];
      hi[q] = h > hi[q] ? h : hi[q];
    }
    if (has_y) spit += 0.5 * erfc(-((y - mu) * ((1.0 / sg) * rsqrt2)));
  }
  if (n == 0 || bad) return;
  const double dn = (double)n;
  if (has_y) *pit = spit / dn;

  // per probability: phase 0 = verifying lo, 1 = verifying hi, 2 = iterating, 3 = finished
  double x[NQ], a[NQ], b[NQ], grow[NQ], wref[NQ], pend[NQ], over[NQ];
  int phase[NQ], stall[NQ], side[NQ];
SGP_MQ_UNROLL
  for (int q = 0; q < NQ; ++q) {
    phase[q] = q < Q ? 0 : 3;
    x[q] = a[q] = lo[q];
    b[q] = hi[q];
    grow[q] = wref[q] = hi[q] - lo[q];  // > 0: at least 2 z sigma_min
    pend[q] = nan, over[q] = 0.25, stall[q] = 0, side[q] = -1;
    if (q < Q && !(grow[q] < inf)) phase[q] = 3;  // a bracket that overflows: NaN
  }
  int it = 0;
  for (;;) {
    bool any = false;
SGP_MQ_UNROLL
    for (int q = 0; q < NQ; ++q) any = any || phase[q] < 3;
    if (!any || it >= MQ_MAX_ITERS) break;
    ++it;
    double sg_[NQ], sd_[NQ];
SGP_MQ_UNROLL
    for (int q = 0; q < NQ; ++q) sg_[q] = sd_[q] = 0.0;
    for (int64_t s = 0; s < n_draws; ++s) {  // one pass: a draw is loaded once for all the probabilities
      if (info[s] != 0) continue;
      const double mu = mean[s * stride];
      const double is = (1.0 / sqrt(var[s * stride])) * rsqrt2;
SGP_MQ_UNROLL
      for (int q = 0; q < NQ; ++q) {
        if (phase[q] < 3) {
          const double u = (x[q] - mu) * is;
          sg_[q] += 0.5 * erfc(pr.upper[q] ? u : -u);
          sd_[q] += exp(-u * u) * is;
        }
      }
    }
SGP_MQ_UNROLL
    for (int q = 0; q < NQ; ++q) {
      if (phase[q] >= 3) continue;
      const double pt = pr.p_tail[q];
      const double tail = sg_[q] / dn, dens = sd_[q] / dn * rsqrtpi;
      if (tail != tail) {  // x overflowed on the way out
        phase[q] = 3;
        continue;
      }
      const bool above = pr.upper[q] ? tail > pt : tail < pt;  // the quantile lies above x
      if (phase[q] == 0) {
        if (above) {
          a[q] = x[q], phase[q] = 1, x[q] = b[q];
          pend[q] = tail;  // (kept for the first point of the iteration)
        } else {  // rounding broke the lower end: step outwards
          x[q] -= grow[q], grow[q] *= 2.0;
        }
        continue;
      }
      if (phase[q] == 1) {
        if (!above) {
          b[q] = x[q], phase[q] = 2;
          wref[q] = b[q] - a[q];
          // the first point: where the line through the two ends' log-tails meets log p_tail, kept off the ends; else the middle
          double f = log(pt / pend[q]) / log(tail / pend[q]);
          f = f > 0.05 ? f : 0.05;
          f = f < 0.95 ? f : 0.95;  // (a NaN falls through both and leaves the bracket in the test below)
          x[q] = a[q] + f * wref[q];
          if (!(x[q] > a[q] && x[q] < b[q])) x[q] = a[q] + 0.5 * wref[q];
          pend[q] = nan;
        } else {  // the upper end: outwards (x is a valid lower end meanwhile)
          a[q] = x[q], pend[q] = tail;
          x[q] += grow[q], grow[q] *= 2.0;
        }
        continue;
      }
      if (above) a[q] = x[q]; else b[q] = x[q];
      over[q] = (int)above == side[q] ? 2.0 * over[q] : 0.25;  // the same side again: push further past the next target
      side[q] = (int)above;
      const double width = b[q] - a[q], mid = a[q] + 0.5 * width;
      if (width <= mq_width(mid, smin)) {
        quant[q] = mid, phase[q] = 3;
        continue;
      }
      if (width <= 0.5 * wref[q]) wref[q] = width, stall[q] = 0;
      double cand = pend[q];
      if (!(cand > a[q] && cand < b[q])) {  // no proposal waits: Newton on log(tail): d/dx log G- = g / G-, d/dx log G+ = -g / G+
        const double step = tail * log(tail / pt) / dens;
        const double delta = pr.upper[q] ? step : -step;
        cand = x[q] + delta;
        cand += copysign(over[q] * mq_width(cand, smin), delta);
        if (!(dens > 0.0 && tail > 0.0 && delta != 0.0 && cand > a[q] && cand < b[q])) cand = nan;  // (a NaN fails them all)
      }
      if (cand == cand && stall[q] < MQ_STALL) {
        x[q] = cand, pend[q] = nan, ++stall[q];
      } else {  // a bisection; a proposal that the stall rule held back is taken up after it
        x[q] = mid, pend[q] = cand;
      }
    }
  }
  *iters = it;
}

}  // namespace sgp
