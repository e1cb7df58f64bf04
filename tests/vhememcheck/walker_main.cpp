// tests/vhememcheck/walker_main.cpp -- TEST-ONLY stand-alone program: the VHEM EM loop's
// shared functions (csrc/vhem_em_trial_ctrl.h, csrc/vhem_em_iter_body.h) on the CPU under
// the address and undefined-behaviour sanitizers (`make vhemem_sanitize`; plain C++, no
// device compiler).  The stopping rule is walked over hand-made likelihood sequences
// with every trial's LogLs in a vector of exactly max_iter + 2 entries, as
// vhem_em_run_trials lays them out; the body runs over every (k, s) of small trials whose
// arrays have exactly the documented sizes, so an access past an end is an error the
// sanitizer reports.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vhem_em_iter_body.h"
#include "vhem_em_trial_ctrl.h"

namespace {

struct Seq {
  const char *name;
  int n;
  double L[12];
  int max_iter, min_iter;
  double termvalue;
  int num_iter;  // the hand-made outcome: num_iter at the stop
};

const double kNaN = std::nan("");
const double kInf = INFINITY;

const Seq kSeqs[] = {
    {"converges", 5, {-100, -90, -89, -88.9, -88.8999}, 20, 1, 1e-5, 4},
    {"no stop at 0 and 1", 3, {-5, -50, -500}, 20, 0, 1e-5, 2},
    {"falling stops", 3, {-100, -90, -95}, 20, 1, 1e-5, 2},
    {"nan runs out", 5, {kNaN, kNaN, kNaN, kNaN, kNaN}, 3, 1, 1e-5, 4},
    {"-inf then finite", 4, {-kInf, -10, -9, -9}, 20, 1, 1e-5, 3},
    {"-inf twice", 5, {-kInf, -kInf, -kInf, -10, -10}, 20, 1, 1e-5, 4},
    {"min_iter 5", 6, {-100, -90, -89.9999999, -89.9999999, -89.9999999, -89.9999999}, 20, 5, 1e-5, 5},
    {"max_iter 0", 2, {-100, -50}, 0, 1, 1e-5, 1},
    {"termvalue 0", 5, {-100, -90, -80, -70, -60}, 3, 1, 0.0, 4},
};

int walk_rule() {
  int bad = 0;
  for (const Seq &s : kSeqs) {
    vhem::TrialCtrl c;
    vhem::trial_ctrl_init(&c);
    std::vector<double> LogLs((size_t)vhem::trial_ctrl_slots(s.max_iter), -7.0);
    int steps = 0;
    while (!c.done && steps < s.n) {
      const double L = s.L[steps];
      const int what = vhem::trial_ctrl_ends(&c, L, s.max_iter, s.min_iter, s.termvalue)
                           ? vhem::kTrialStop : vhem::kTrialContinue;
      const int slot = vhem::trial_ctrl_record(&c, what, L, steps);
      bad += slot != steps;
      LogLs[(size_t)slot] = L;  // a slot past max_iter + 2 is the sanitizer's to report
      ++steps;
    }
    std::printf("%-20s steps=%d num_iter=%d done=%d stop_iter=%d\n", s.name, steps, c.num_iter, c.done,
                c.stop_iter);
    bad += !c.done || steps != s.n || c.num_iter != s.num_iter || c.stop_iter != steps - 1 ||
           c.fallback || steps > s.max_iter + 2;
  }
  // the device's decision: a likelihood that is not finite is a fallback
  vhem::TrialCtrl c;
  vhem::trial_ctrl_init(&c);
  bad += vhem::trial_ctrl_decide(&c, kNaN, 5, 1, 1e-5) != vhem::kTrialFallback;
  bad += vhem::trial_ctrl_decide(&c, -kInf, 5, 1, 1e-5) != vhem::kTrialFallback;
  bad += vhem::trial_ctrl_decide(&c, -3.0, 5, 1, 1e-5) != vhem::kTrialContinue;
  return bad;
}

// a small deterministic trial: statistics of K S well-conditioned states
int walk_body(int K, int S, int d, int covmode, int tau, int zero_cluster) {
  const int NU = covmode == 1 ? 1 + d + d * (d + 1) / 2 : 1 + 2 * d, KS = K * S;
  const int dd = covmode == 1 ? d * d : d;
  std::vector<double> st((size_t)K + KS + (size_t)KS * S + 2 + (size_t)KS * NU);
  double *Nj = st.data(), *N1 = Nj + K, *M = N1 + KS, *U = M + (size_t)KS * S + 2;
  unsigned seed = 12345u + (unsigned)(K * 131 + S * 17 + d);
  auto rnd = [&seed]() {
    seed = seed * 1664525u + 1013904223u;
    return 0.25 + (double)(seed >> 8) / (double)(1u << 24);
  };
  for (int k = 0; k < K; ++k) Nj[k] = k == zero_cluster ? 0.0 : 2.0 + rnd();
  for (int x = 0; x < KS; ++x) N1[x] = rnd();
  for (int x = 0; x < KS * S; ++x) M[x] = rnd();
  M[(size_t)KS * S] = -123.5;
  for (int x = 0; x < KS; ++x) {
    double *u = U + (size_t)x * NU;
    const double w = 3.0 + rnd();
    u[0] = w;
    std::vector<double> mu((size_t)d);
    for (int q = 0; q < d; ++q) {
      mu[(size_t)q] = rnd() - 0.7;
      u[1 + q] = w * mu[(size_t)q];
    }
    if (covmode == 1) {
      int o = 1 + d;
      for (int r = 0; r < d; ++r)
        for (int c = r; c < d; ++c)
          u[o++] = w * ((r == c ? 1.0 + 0.1 * r : 0.05) + mu[(size_t)r] * mu[(size_t)c]);
    } else {
      for (int q = 0; q < d; ++q) u[1 + d + q] = w * (1.0 + 0.1 * q + mu[(size_t)q] * mu[(size_t)q]);
    }
  }
  std::vector<double> omega((size_t)K), prior((size_t)KS), A((size_t)KS * S), cen((size_t)KS * d),
      cov((size_t)KS * dd), vc((size_t)KS), logA((size_t)KS * S), logPi((size_t)KS), cm((size_t)KS * d),
      P((size_t)KS * dd), c((size_t)KS), logOmega((size_t)K);
  vhem::KsArgs a{};
  a.K = K; a.S = S; a.d = d; a.covmode = covmode; a.NU = NU; a.Kb = 7; a.tau = tau; a.reg_cov = 0.001;
  a.stats = st.data();
  a.omega = omega.data(); a.prior = prior.data(); a.A = A.data(); a.centres = cen.data();
  a.covars = cov.data(); a.vcounts = vc.data();
  a.logA = logA.data(); a.logPi = logPi.data(); a.cm = cm.data(); a.P = P.data(); a.c = c.data();
  a.logOmega = logOmega.data();
  std::vector<double> g((size_t)2 * d * d);
  const vhem::HostWave w;
  int flag = 0;
  for (int ks = 0; ks < KS; ++ks) flag |= vhem::vhem_ks_body(a, ks, w, g.data());
  int bad = flag != (zero_cluster >= 0);
  // the prelude of what the M-step wrote gives the same constants (omega == 0 passes there)
  std::vector<double> c2((size_t)KS), P2((size_t)KS * dd);
  a.stats = nullptr;
  a.c = c2.data();
  a.P = P2.data();
  int flag2 = 0;
  for (int ks = 0; ks < KS; ++ks) flag2 |= vhem::vhem_ks_body(a, ks, w, g.data());
  bad += flag2 != 0;
  for (int x = 0; x < KS; ++x) bad += !(c2[(size_t)x] == c[(size_t)x]);
  for (int x = 0; x < KS * dd; ++x) bad += !(P2[(size_t)x] == P[(size_t)x]);
  // P cov = I
  if (covmode == 1)
    for (int x = 0; x < KS; ++x)
      for (int r = 0; r < d; ++r)
        for (int q = 0; q < d; ++q) {
          double sum = 0.0;
          for (int m = 0; m < d; ++m) sum += P[(size_t)x * dd + r * d + m] * cov[(size_t)x * dd + m * d + q];
          bad += !(std::fabs(sum - (r == q ? 1.0 : 0.0)) < 1e-10);
        }
  std::printf("body K=%d S=%d d=%d cov=%d tau=%d zero=%d: flag=%d prelude flag=%d\n", K, S, d, covmode, tau,
              zero_cluster, flag, flag2);
  return bad;
}

}  // namespace

int main() {
  int bad = walk_rule();
  const int ds[] = {1, 2, 8, 16}, Ss[] = {1, 3, 16};
  for (int covmode = 0; covmode <= 1; ++covmode)
    for (int d : ds)
      for (int S : Ss) bad += walk_body(2, S, d, covmode, 6, -1);
  bad += walk_body(3, 3, 2, 1, 1, -1);
  bad += walk_body(3, 3, 2, 1, 6, 1);
  std::printf("vhemem walker: %d errors\n", bad);
  return bad ? 1 : 0;
}
