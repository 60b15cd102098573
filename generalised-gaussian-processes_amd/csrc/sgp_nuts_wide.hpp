// NUTS for WIDE positions -- the sampler of the joint model (all_in_HMC: hyper-parameters AND inducing inputs, ndim =
// d + 2 + M d, up to 3 098).  Same algorithm, same random stream and the same resumable state machine as sgp_nuts.hpp
// (multinomial NUTS, generalised U-turn on sub-trees, dual averaging, PyMC3's jitter+adapt_diag mass adaptation; see there
// and hmc.py), but:
//   * ndim is a run-time value and every vector lives in a caller-provided workspace (WideWs): points, the sub-tree stack's
//     momenta and p_sum, the mass adapter's windows.  Only scalars stay in the state (LDS on the GPU);
//   * the WN_LANES = 256 threads of one workgroup call wnuts_step together: thread t owns the entries i = t, t + 256, ...
//     of every vector (element-wise updates need no barrier: a thread only ever reads entries it wrote itself) and thread 0
//     alone writes the scalar state, between barriers;
//   * dot products use ONE fixed reduction order, on the device and in the host build alike (wn_reduce): lane t sums its
//     entries in increasing i, each wave of 64 lanes is folded by the tree v[t] += v[t + h], h = 32, 16, ..., 1, and the four
//     wave sums are combined as (w0 + w1) + (w2 + w3);
//   * the momentum is drawn in parallel: splitmix64 is a counter generator, so normal k of the draw is computed from the
//     state at the start of it (Box-Muller pairs, the spare of the previous draw first) -- the same numbers, in the same
//     order, as hmc.SplitMix.standard_normal;
//   * sub-tree proposals (q, grad) live in a pool of WN_SLOTS slots and are tracked by reference-counted slot index: a merge
//     or an accepted proposal moves an index, never a vector.
// The host build (g++, one "thread": tid 0, stride 1, barriers empty) is what the CPU tests run against hmc.NUTS.
#pragma once
#include "sgp_nuts.hpp"

namespace sgp {

constexpr int WN_LANES = 256;
constexpr int WN_SLOTS = 20;  // cur, left, right, edge, top proposal, trial + one per sub-tree stack level (<= 12): 18 at most
enum { WN_RED_MAX = 6 };      // values reduced in one pass (the three U-turn checks of a merge: six dot products)

#if defined(__HIP_DEVICE_COMPILE__)
#define WN_SYNC() __syncthreads()
#define WN_STRIDE WN_LANES
#else
#define WN_SYNC() ((void)0)
#define WN_STRIDE 1
#endif
#define WN_FOR(i, n) for (int i = tid; i < (n); i += WN_STRIDE)
// No fused multiply-adds in the sampler's arithmetic (first statement of every function that computes): the device then rounds
// like the host build (g++ -ffp-contract=off) and hmc.NUTS.  Scoped to those bodies: the code that includes this header keeps its own
// contraction.
#if defined(__clang__)
#define WN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define WN_NO_CONTRACT
#endif

struct WideWs {  // vectors of ndim doubles each (wide_ws_doubles(ndim) in all)
  double *var, *wv_mean[2], *wv_m2[2];  // inverse metric ; the mass adapter's two windows (fg = wv[fg_sel])
  double *p_cur, *p_left, *p_right, *p_edge, *p_trial;
  double *top_psum, *tmp[3];
  double *stk_lp, *stk_rp, *stk_psum;   // NUTS_MAXDEPTH x ndim each
  double *slot_q, *slot_g;              // WN_SLOTS x ndim each
};
SGP_HD inline size_t wide_ws_doubles(int n) { return (size_t)n * (5 + 5 + 4 + 3 * NUTS_MAXDEPTH + 2 * WN_SLOTS); }
SGP_HD inline WideWs wide_ws_carve(double* base, int n) {
  WideWs w;
  double* p = base;
  auto take = [&](int k) { double* r = p; p += (size_t)k * n; return r; };
  w.var = take(1);
  for (int k = 0; k < 2; ++k) { w.wv_mean[k] = take(1); w.wv_m2[k] = take(1); }
  w.p_cur = take(1); w.p_left = take(1); w.p_right = take(1); w.p_edge = take(1); w.p_trial = take(1);
  w.top_psum = take(1);
  for (int k = 0; k < 3; ++k) w.tmp[k] = take(1);
  w.stk_lp = take(NUTS_MAXDEPTH); w.stk_rp = take(NUTS_MAXDEPTH); w.stk_psum = take(NUTS_MAXDEPTH);
  w.slot_q = take(WN_SLOTS); w.slot_g = take(WN_SLOTS);
  return w;
}

struct WideTree {  // a finished sub-tree: its vectors are row `level` of stk_* ; the proposal is a slot
  int prop, n, depth, diverging, turning;
  double prop_logp, prop_energy, log_size, accept_sum;
};

struct WideState {
  int ndim, n_tune, n_draws, max_treedepth;
  double target_accept, Emax;
  double da_mu, da_log_step, da_log_bar, da_hbar, da_gamma, da_t0, da_kappa;
  int da_count;
  double wv_n[2];  // weights of the two windows
  int fg_sel, mass_count, mass_window;
  NutsRng rng;
  int phase, it;
  long n_leapfrog;
  // points: slot of (q, grad) + the momentum vector of the same name
  int s_cur, s_left, s_right, s_edge, s_trial;
  double cur_logp, cur_energy, trial_logp, trial_energy;
  double eps, e0;
  int s_top;  // top-level proposal
  double top_prop_logp, top_prop_energy, top_log_size, top_accept_sum;
  int top_n, depth, direction, diverging, nleaf, nleaf_target, sp;
  int bflag;     // a branch decision broadcast by thread 0
  int slot_overflow;  // set by wn_alloc if the slot pool were ever exhausted
  WideTree stack[NUTS_MAXDEPTH];
  int refc[WN_SLOTS];
  double red[WN_RED_MAX][4];  // wave sums of wn_reduce
};

// ---- slot bookkeeping (thread 0 only) ----------------------------------------------------------------------------
SGP_HD inline void wn_ref(WideState& s, int slot) { if (slot >= 0) s.refc[slot] += 1; }
SGP_HD inline void wn_unref(WideState& s, int& holder) {
  if (holder >= 0) s.refc[holder] -= 1;
  holder = -1;
}
SGP_HD inline void wn_set(WideState& s, int& holder, int slot) {  // holder := slot (ref first: holder may already be slot)
  wn_ref(s, slot);
  wn_unref(s, holder);
  holder = slot;
}
SGP_HD inline int wn_alloc(WideState& s) {
  for (int k = 0; k < WN_SLOTS; ++k)
    if (s.refc[k] == 0) return k;
  s.slot_overflow = 1;  // cannot happen (at most 18 slots are held at once); the host build's callers check the flag
  return 0;
}
SGP_HD inline double* wn_q(const WideWs& w, const WideState& s, int slot) { return w.slot_q + (size_t)slot * s.ndim; }
SGP_HD inline double* wn_g(const WideWs& w, const WideState& s, int slot) { return w.slot_g + (size_t)slot * s.ndim; }

// ---- the fixed-order reduction -----------------------------------------------------------------------------------
// term(i, v) adds the contributions of entry i to v[0..K-1]; every thread returns the K totals in out[].
template <int K, class F>
SGP_HD inline void wn_reduce(WideState& s, int tid, int n, F term, double (&out)[K]) {
  WN_NO_CONTRACT
#if defined(__HIP_DEVICE_COMPILE__)
  double v[K];
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  for (int i = tid; i < n; i += WN_LANES) term(i, v);
  const int lane = tid & 63, wv = tid >> 6;
  for (int h = 32; h >= 1; h >>= 1)
    for (int k = 0; k < K; ++k) {
      const double o = __shfl_down(v[k], h, 64);
      if (lane < h) v[k] += o;
    }
  __syncthreads();  // the previous reduction's totals have been read by every thread
  if (lane == 0)
    for (int k = 0; k < K; ++k) s.red[k][wv] = v[k];
  __syncthreads();
  for (int k = 0; k < K; ++k) out[k] = (s.red[k][0] + s.red[k][1]) + (s.red[k][2] + s.red[k][3]);
#else
  (void)tid;
  double lanev[WN_LANES][K];
  for (int t = 0; t < WN_LANES; ++t) {
    for (int k = 0; k < K; ++k) lanev[t][k] = 0.0;
    for (int i = t; i < n; i += WN_LANES) term(i, lanev[t]);
  }
  double ws[4][K];
  for (int wv = 0; wv < 4; ++wv) {
    double* b = &lanev[64 * wv][0];
    for (int h = 32; h >= 1; h >>= 1)
      for (int t = 0; t < h; ++t)
        for (int k = 0; k < K; ++k) b[t * K + k] += b[(t + h) * K + k];
    for (int k = 0; k < K; ++k) ws[wv][k] = b[k];
  }
  for (int k = 0; k < K; ++k) out[k] = (ws[0][k] + ws[1][k]) + (ws[2][k] + ws[3][k]);
  (void)s;
#endif
}

// kinetic energy 0.5 p . (var o p)
SGP_HD inline double wn_kinetic(WideState& s, const WideWs& w, int tid, const double* p) {
  WN_NO_CONTRACT
  double r[1];
  wn_reduce<1>(s, tid, s.ndim, [&](int i, double* v) { v[0] += p[i] * (w.var[i] * p[i]); }, r);
  return 0.5 * r[0];
}

// ---- momentum: n normals of the SplitMix stream, in parallel ------------------------------------------------------
SGP_HD inline uint64_t wn_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
SGP_HD inline void wn_pair(uint64_t s0, long j, double& c, double& sn) {  // Box-Muller pair j from state s0
  WN_NO_CONTRACT
  const uint64_t a = wn_mix(s0 + (uint64_t)(2 * j + 1) * 0x9E3779B97F4A7C15ull);
  const uint64_t b = wn_mix(s0 + (uint64_t)(2 * j + 2) * 0x9E3779B97F4A7C15ull);
  const double u1 = 1.0 - (double)(a >> 11) * (1.0 / 9007199254740992.0), u2 = (double)(b >> 11) * (1.0 / 9007199254740992.0);
  const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
  c = rad * cos(ang);
  sn = rad * sin(ang);
}
// p[i] = normal_i / sqrt(var[i]); the generator is advanced past the n normals by thread 0 (caller: barrier afterwards)
SGP_HD inline void wn_momentum(WideState& s, const WideWs& w, int tid, double* p) {
  WN_NO_CONTRACT
  const int n = s.ndim;
  const uint64_t s0 = s.rng.s;
  const int hs = s.rng.have_spare;
  const double spare = s.rng.spare;
  WN_FOR(i, n) {
    double z;
    if (hs && i == 0) {
      z = spare;
    } else {
      const long k = i - hs;
      double c, sn;
      wn_pair(s0, k >> 1, c, sn);
      z = (k & 1) ? sn : c;
    }
    p[i] = z / sqrt(w.var[i]);
  }
  WN_SYNC();  // every thread has read the generator's state
  if (tid == 0) {
    const long m = n - hs, pairs = (m + 1) / 2;
    if (m & 1) {
      double c, sn;
      wn_pair(s0, pairs - 1, c, sn);
      s.rng.spare = sn;
      s.rng.have_spare = 1;
    } else {
      s.rng.have_spare = 0;
    }
    s.rng.s = s0 + (uint64_t)(2 * pairs) * 0x9E3779B97F4A7C15ull;
  }
}

// q_start: where the chain starts (PyMC3's jitter already added).  All threads call it; barrier afterwards.
SGP_HD inline void wnuts_init(WideState& s, const WideWs& w, int tid, int ndim, int n_tune, int n_draws, int max_treedepth,
                              double step_scale, double target_accept, uint64_t seed, const double* q_start) {
  WN_NO_CONTRACT
  WN_FOR(i, ndim) {
    w.var[i] = 1.0;
    w.wv_mean[0][i] = q_start[i];
    w.wv_m2[0][i] = 1.0 * 10.0;
    w.wv_mean[1][i] = 0.0;
    w.wv_m2[1][i] = 0.0;
    w.slot_q[i] = q_start[i];  // slot 0 = the current state
  }
  if (tid == 0) {
    s.ndim = ndim;
    s.n_tune = n_tune;
    s.n_draws = n_draws;
    s.max_treedepth = max_treedepth;
    s.target_accept = target_accept;
    s.Emax = 1000.0;
    const double step0 = step_scale / pow((double)ndim, 0.25);
    s.da_mu = log(10.0 * step0);
    s.da_log_step = log(step0);
    s.da_log_bar = log(step0);
    s.da_hbar = 0.0;
    s.da_gamma = 0.05;
    s.da_t0 = 10.0;
    s.da_kappa = 0.75;
    s.da_count = 1;
    s.wv_n[0] = 10.0;
    s.wv_n[1] = 0.0;
    s.fg_sel = 0;
    s.mass_count = 0;
    s.mass_window = 101;
    s.rng.s = seed;
    s.rng.have_spare = 0;
    s.rng.spare = 0.0;
    s.phase = NS_INIT;
    s.it = 0;
    s.n_leapfrog = 0;
    for (int k = 0; k < WN_SLOTS; ++k) s.refc[k] = 0;
    s.slot_overflow = 0;
    s.s_cur = s.s_left = s.s_right = s.s_edge = s.s_trial = s.s_top = -1;
    wn_set(s, s.s_cur, 0);
    s.sp = 0;
  }
  WN_SYNC();
}

// the half step from the edge in s.direction: trial (a fresh slot) gets q, p_trial the half-step momentum, qpub the position
SGP_HD inline void wn_half_step(WideState& s, const WideWs& w, int tid, double* qpub) {
  WN_NO_CONTRACT
  WN_SYNC();
  if (tid == 0) wn_set(s, s.s_trial, wn_alloc(s));
  WN_SYNC();
  const double e = s.eps * (double)s.direction;
  const double *eq = wn_q(w, s, s.s_edge), *eg = wn_g(w, s, s.s_edge);
  double* tq = wn_q(w, s, s.s_trial);
  WN_FOR(i, s.ndim) {
    const double ph = w.p_edge[i] + 0.5 * e * eg[i];
    w.p_trial[i] = ph;
    const double q = eq[i] + e * (w.var[i] * ph);
    tq[i] = q;
    qpub[i] = q;
  }
}

SGP_HD inline void wn_begin_doubling(WideState& s, const WideWs& w, int tid, double* qpub) {
  WN_SYNC();
  if (tid == 0) {
    s.direction = rng_uniform(s.rng) < 0.5 ? 1 : -1;
    wn_set(s, s.s_edge, s.direction > 0 ? s.s_right : s.s_left);
    s.sp = 0;
    s.nleaf = 0;
    s.nleaf_target = 1 << s.depth;
  }
  WN_SYNC();
  const double* src = s.direction > 0 ? w.p_right : w.p_left;
  WN_FOR(i, s.ndim) w.p_edge[i] = src[i];
  wn_half_step(s, w, tid, qpub);
}

// merge stack level b = a + 1 into a (sgp_nuts.hpp: nuts_merge)
SGP_HD inline void wn_merge(WideState& s, const WideWs& w, int tid, int la) {
  WN_NO_CONTRACT
  const int n = s.ndim, lb = la + 1;
  WN_SYNC();
  WideTree& a = s.stack[la];
  WideTree& b = s.stack[lb];
  const bool bad = b.diverging || b.turning;
  double* psum = w.tmp[0];
  double *apsum = w.stk_psum + (size_t)la * n, *bpsum = w.stk_psum + (size_t)lb * n;
  double *alp = w.stk_lp + (size_t)la * n, *blp = w.stk_lp + (size_t)lb * n;
  double *arp = w.stk_rp + (size_t)la * n, *brp = w.stk_rp + (size_t)lb * n;
  WN_FOR(i, n) psum[i] = apsum[i] + bpsum[i];
  int turning = b.turning;
  if (!bad) {
    const bool fwd = s.direction > 0;
    const double *f_psum = fwd ? apsum : bpsum, *f_lp = fwd ? alp : blp, *f_rp = fwd ? arp : brp;
    const double *s_psum = fwd ? bpsum : apsum, *s_lp = fwd ? blp : alp, *s_rp = fwd ? brp : arp;
    double r[6];
    wn_reduce<6>(s, tid, n, [&](int i, double* v) {
      const double t1 = f_psum[i] + s_lp[i], t2 = f_rp[i] + s_psum[i];
      v[0] += psum[i] * (w.var[i] * f_lp[i]);
      v[1] += psum[i] * (w.var[i] * s_rp[i]);
      v[2] += t1 * (w.var[i] * f_lp[i]);
      v[3] += t1 * (w.var[i] * s_lp[i]);
      v[4] += t2 * (w.var[i] * f_rp[i]);
      v[5] += t2 * (w.var[i] * s_rp[i]);
    }, r);
    turning = (r[0] <= 0.0 || r[1] <= 0.0) || (r[2] <= 0.0 || r[3] <= 0.0) || (r[4] <= 0.0 || r[5] <= 0.0);
  }
  if (s.direction > 0) {
    WN_FOR(i, n) arp[i] = brp[i];
  } else {
    WN_FOR(i, n) alp[i] = blp[i];
  }
  WN_FOR(i, n) apsum[i] = psum[i];
  WN_SYNC();
  if (tid == 0) {
    const double log_size = nuts_logaddexp(a.log_size, b.log_size);
    bool take_b = false;
    if (!bad) take_b = log(rng_uniform(s.rng) + 1e-300) < b.log_size - log_size;
    if (take_b) {
      wn_set(s, a.prop, b.prop);
      a.prop_logp = b.prop_logp;
      a.prop_energy = b.prop_energy;
    }
    wn_unref(s, b.prop);
    a.log_size = log_size;
    a.accept_sum += b.accept_sum;
    a.n += b.n;
    a.depth += 1;
    a.diverging = b.diverging;
    a.turning = turning;
  }
  WN_SYNC();
}

// One call by all threads = everything the sampler can do without a new evaluation (sgp_nuts.hpp: nuts_step).  On entry
// (except the first call) logp (the same value in every thread) and grad[ndim] are the target at the last published
// position.  Returns NUTS_EVAL with the next position written to qpub[ndim], or NUTS_DONE.  samples: n_draws x ndim,
// stats: n_draws x NST_COLS.
SGP_HD inline int wnuts_step(WideState& s, const WideWs& w, int tid, double logp, const double* grad, double* qpub, double* samples,
                             double* stats) {
  WN_NO_CONTRACT
  const int n = s.ndim;
  WN_SYNC();
  if (s.phase == NS_INIT) {
    const double* q = wn_q(w, s, s.s_cur);
    WN_FOR(i, n) qpub[i] = q[i];
    WN_SYNC();
    if (tid == 0) s.phase = NS_WAIT_INIT;
    WN_SYNC();
    return NUTS_EVAL;
  }
  if (s.phase == NS_WAIT_INIT) {
    double* g = wn_g(w, s, s.s_cur);
    WN_FOR(i, n) g[i] = grad[i];
    WN_SYNC();
    if (tid == 0) {
      s.n_leapfrog += 1;
      s.cur_logp = logp;
      s.phase = isfinite(logp) ? NS_BEGIN_DRAW : NS_FINISHED;
    }
    WN_SYNC();
    if (s.phase == NS_FINISHED) return NUTS_DONE;
  }
  for (;;) {
    if (s.phase == NS_BEGIN_DRAW) {
      if (s.it >= s.n_tune + s.n_draws) {
        WN_SYNC();
        if (tid == 0) s.phase = NS_FINISHED;
        WN_SYNC();
        return NUTS_DONE;
      }
      WN_SYNC();
      if (tid == 0) s.eps = exp(s.it < s.n_tune ? s.da_log_step : s.da_log_bar);
      wn_momentum(s, w, tid, w.p_cur);
      const double kin = wn_kinetic(s, w, tid, w.p_cur);
      WN_FOR(i, n) {
        const double p = w.p_cur[i];
        w.p_left[i] = p;
        w.p_right[i] = p;
        w.top_psum[i] = p;
      }
      WN_SYNC();
      if (tid == 0) {
        s.cur_energy = isfinite(s.cur_logp) ? -s.cur_logp + kin : INFINITY;
        s.e0 = s.cur_energy;
        wn_set(s, s.s_left, s.s_cur);
        wn_set(s, s.s_right, s.s_cur);
        wn_set(s, s.s_top, s.s_cur);
        s.top_prop_logp = s.cur_logp;
        s.top_prop_energy = s.cur_energy;
        s.top_log_size = 0.0;
        s.top_accept_sum = 0.0;
        s.top_n = 0;
        s.depth = 0;
        s.diverging = 0;
        s.phase = NS_WAIT_LEAF;
      }
      WN_SYNC();
      if (s.depth >= s.max_treedepth) goto end_draw;
      wn_begin_doubling(s, w, tid, qpub);
      WN_SYNC();
      return NUTS_EVAL;
    }
    if (s.phase == NS_WAIT_LEAF) {
      // ---- finish the leapfrog and make the leaf ------------------------------------------------------------------
      double fin[1];
      wn_reduce<1>(s, tid, n, [&](int i, double* v) { v[0] += isfinite(grad[i]) ? 0.0 : 1.0; }, fin);
      const bool finite = isfinite(logp) && fin[0] == 0.0;
      const double e = s.eps * (double)s.direction;
      double* tg = wn_g(w, s, s.s_trial);
      const int lv = s.sp;
      double *lp_ = w.stk_lp + (size_t)lv * n, *rp_ = w.stk_rp + (size_t)lv * n, *ps_ = w.stk_psum + (size_t)lv * n;
      if (finite) {
        WN_FOR(i, n) {
          w.p_trial[i] += 0.5 * e * grad[i];
          tg[i] = grad[i];
        }
      } else {
        WN_FOR(i, n) tg[i] = 0.0;
      }
      const double kin = finite ? wn_kinetic(s, w, tid, w.p_trial) : 0.0;
      WN_FOR(i, n) {
        const double p = w.p_trial[i];
        w.p_edge[i] = p;
        lp_[i] = p;
        rp_[i] = p;
        ps_[i] = p;
      }
      WN_SYNC();
      if (tid == 0) {
        s.n_leapfrog += 1;
        s.trial_logp = finite ? logp : -INFINITY;
        s.trial_energy = finite ? -logp + kin : INFINITY;
        wn_set(s, s.s_edge, s.s_trial);
        WideTree& t = s.stack[s.sp];
        double de = s.trial_energy - s.e0;
        if (!isfinite(de)) de = INFINITY;
        t.prop = -1;
        wn_set(s, t.prop, s.s_trial);
        wn_unref(s, s.s_trial);
        t.prop_logp = s.trial_logp;
        t.prop_energy = s.trial_energy;
        t.diverging = de > s.Emax;
        t.log_size = isfinite(de) ? -de : -INFINITY;
        t.accept_sum = (de > -700.0 && isfinite(de)) ? fmin(1.0, exp(-de)) : (de <= -700.0 ? 1.0 : 0.0);
        t.n = 1;
        t.depth = 0;
        t.turning = 0;
        s.sp += 1;
        s.nleaf += 1;
      }
      WN_SYNC();
      // ---- binary-counter merging ---------------------------------------------------------------------------------
      bool bad = s.stack[s.sp - 1].diverging || s.stack[s.sp - 1].turning;
      while (!bad && s.sp >= 2 && s.stack[s.sp - 2].depth == s.stack[s.sp - 1].depth) {
        wn_merge(s, w, tid, s.sp - 2);
        if (tid == 0) s.sp -= 1;
        WN_SYNC();
        bad = s.stack[s.sp - 1].diverging || s.stack[s.sp - 1].turning;
      }
      if (bad) {
        while (s.sp >= 2) {
          wn_merge(s, w, tid, s.sp - 2);
          if (tid == 0) s.sp -= 1;
          WN_SYNC();
        }
      } else if (s.nleaf < s.nleaf_target) {
        wn_half_step(s, w, tid, qpub);
        WN_SYNC();
        return NUTS_EVAL;
      }
      // ---- the sub-tree is finished: top level of NUTS.draw ---------------------------------------------------------
      WN_SYNC();
      if (tid == 0) {
        WideTree& sub = s.stack[0];
        s.top_accept_sum += sub.accept_sum;
        s.top_n += sub.n;
        s.bflag = sub.diverging ? 1 : (sub.turning ? 2 : 0);
        if (sub.diverging) s.diverging = 1;
        if (!s.bflag) {
          if (log(rng_uniform(s.rng) + 1e-300) < sub.log_size - s.top_log_size) {
            wn_set(s, s.s_top, sub.prop);
            s.top_prop_logp = sub.prop_logp;
            s.top_prop_energy = sub.prop_energy;
          }
          s.top_log_size = nuts_logaddexp(s.top_log_size, sub.log_size);
          if (s.direction > 0) wn_set(s, s.s_right, s.s_edge);
          else wn_set(s, s.s_left, s.s_edge);
          s.depth += 1;
        }
        wn_unref(s, sub.prop);
        s.sp = 0;
      }
      WN_SYNC();
      if (s.bflag) goto end_draw;
      {
        double* dst = s.direction > 0 ? w.p_right : w.p_left;
        const double* sps = w.stk_psum;  // level 0
        WN_FOR(i, n) {
          dst[i] = w.p_edge[i];
          w.top_psum[i] += sps[i];
        }
        double r[2];
        wn_reduce<2>(s, tid, n, [&](int i, double* v) {
          v[0] += w.top_psum[i] * (w.var[i] * w.p_left[i]);
          v[1] += w.top_psum[i] * (w.var[i] * w.p_right[i]);
        }, r);
        if (r[0] <= 0.0 || r[1] <= 0.0) goto end_draw;
        if (s.depth >= s.max_treedepth) goto end_draw;
        wn_begin_doubling(s, w, tid, qpub);
        WN_SYNC();
        return NUTS_EVAL;
      }
    }
  end_draw : {
    WN_SYNC();
    const bool tuning = s.it < s.n_tune;
    const double accept = s.top_accept_sum / (double)(s.top_n > 1 ? s.top_n : 1);
    const double* pq = wn_q(w, s, s.s_top);
    if (!tuning) {
      const int row = s.it - s.n_tune;
      WN_FOR(i, n) samples[(long)row * n + i] = pq[i];
      if (tid == 0) {
        double* st = stats + (long)row * NST_COLS;
        st[NST_STEP] = s.eps;
        st[NST_TREE] = (double)s.top_n;
        st[NST_DEPTH] = (double)s.depth;
        st[NST_ACCEPT] = accept;
        st[NST_DIVERGING] = (double)s.diverging;
        st[NST_ENERGY] = s.top_prop_energy;
        st[NST_LOGP] = s.top_prop_logp;
        st[NST_NLEAP] = (double)s.n_leapfrog;
      }
    } else {
      // hmc.py: DiagMassAdapter.update (the windows' weights are scalars: every thread computes the new ones)
      const int fg = s.fg_sel, bg = 1 - fg;
      const double nf = s.wv_n[fg] + 1.0, nb = s.wv_n[bg] + 1.0;
      WN_FOR(i, n) {
        const double x = pq[i];
        double d = x - w.wv_mean[fg][i];
        w.wv_mean[fg][i] += d / nf;
        w.wv_m2[fg][i] += d * (x - w.wv_mean[fg][i]);
        d = x - w.wv_mean[bg][i];
        w.wv_mean[bg][i] += d / nb;
        w.wv_m2[bg][i] += d * (x - w.wv_mean[bg][i]);
      }
      double bad[1];
      wn_reduce<1>(s, tid, n, [&](int i, double* v) {
        const double vv = w.wv_m2[fg][i] / nf;
        v[0] += (isfinite(vv) && vv > 0.0) ? 0.0 : 1.0;
      }, bad);
      if (bad[0] == 0.0) WN_FOR(i, n) w.var[i] = w.wv_m2[fg][i] / nf;
      const bool swap = s.mass_count > 0 && s.mass_count % s.mass_window == 0;
      if (swap) WN_FOR(i, n) {  // fg := bg ; the old foreground's buffers become the new, empty background
        w.wv_mean[fg][i] = 0.0;
        w.wv_m2[fg][i] = 0.0;
      }
      WN_SYNC();
      if (tid == 0) {
        const double wd = 1.0 / ((double)s.da_count + s.da_t0);  // hmc.py: DualAveraging.update
        s.da_hbar = (1.0 - wd) * s.da_hbar + wd * (s.target_accept - accept);
        s.da_log_step = s.da_mu - s.da_hbar * sqrt((double)s.da_count) / s.da_gamma;
        const double mk = pow((double)s.da_count, -s.da_kappa);
        s.da_log_bar = mk * s.da_log_step + (1.0 - mk) * s.da_log_bar;
        s.da_count += 1;
        s.wv_n[fg] = nf;
        s.wv_n[bg] = nb;
        if (swap) {
          s.fg_sel = bg;
          s.wv_n[fg] = 0.0;
        }
        s.mass_count += 1;
      }
    }
    WN_SYNC();
    if (tid == 0) {
      wn_set(s, s.s_cur, s.s_top);
      s.cur_logp = s.top_prop_logp;
      wn_unref(s, s.s_top);
      wn_unref(s, s.s_left);
      wn_unref(s, s.s_right);
      wn_unref(s, s.s_edge);
      s.it += 1;
      s.phase = NS_BEGIN_DRAW;
    }
    WN_SYNC();
  }
  }
}

}  // namespace sgp
