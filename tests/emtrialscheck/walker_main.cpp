// tests/emtrialscheck/walker_main.cpp -- TEST-ONLY stand-alone program: the stopping rule
// of one EM trial (csrc/vbhem_em_trial_ctrl.h) driven over the hand-made bound sequences of
// tests/checklib/em_trial_seqs.h (the ones tests/test_em_trials_ctrl.py uses), for a run
// under the address and undefined-behaviour sanitizers on the CPU (`make
// emtrials_sanitize`; plain C++, no device compiler).  Every trial's bounds go into a
// vector of exactly max_iter + 1 entries, as vbhem_em_run_trials lays them out, so a slot
// past the end is an error the sanitizer reports; the outcome is compared with the
// sequence's hand-made one.
#include <cmath>
#include <cstdio>
#include <vector>

#include "em_trial_seqs.h"
#include "vbhem_em_trial_ctrl.h"

int main() {
  int count = 0, bad = 0;
  const emtrialseqs::Seq *seqs = emtrialseqs::table(&count);
  for (int i = 0; i < count; ++i) {
    const emtrialseqs::Seq &s = seqs[i];
    vbhem::TrialCtrl c;
    vbhem::trial_ctrl_init(&c);
    std::vector<double> LogLs((size_t)s.max_iter + 1, -7.0);
    int steps = 0, flips = 0;
    while (!c.done && steps < s.n) {
      const int cur = c.cur;
      const double L = s.L[steps];
      const int slot = vbhem::trial_ctrl_step(&c, L, s.max_iter, s.minDiff);
      if (slot >= 0) LogLs[(size_t)slot] = L;
      bad += slot >= 0 ? slot != steps : !std::isnan(L);  // a running trial's slot is the iteration
      flips += c.cur != cur;
      ++steps;
    }
    std::printf("%-26s steps=%d iters=%d stable=%d done=%d stop_iter=%d cur=%d L_final=%g\n", s.name, steps,
                c.it, c.stable, c.done, c.stop_iter, c.cur, c.L_final);
    bad += !c.done || steps != s.n || c.it != s.iters || c.stable != s.stable || flips != c.it ||
           c.cur != (c.it & 1) || c.stop_iter != steps - 1;
    for (int q = 0; q <= s.max_iter; ++q) {
      const double want = q < c.it ? s.L[q] : -7.0;
      bad += !(LogLs[(size_t)q] == want);
    }
    if (c.stable) bad += !(c.L_final == s.L[steps - 1]) || c.lastL != c.L_final;
    else bad += !(std::isinf(c.L_final) && c.L_final < 0);
  }
  std::printf("emtrials walker: %d sequences, %d errors\n", count, bad);
  return bad ? 1 : 0;
}
