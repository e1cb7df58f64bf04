// tests/emtrialscheck/emtrialscheck.hip -- TEST-ONLY exports of the stopping rule of one
// EM trial (csrc/vbhem_em_trial_ctrl.h), the host build of the function the batched-trials
// kernel runs on the device, and of the hand-made bound sequences
// (tests/checklib/em_trial_seqs.h), so tests/test_em_trials_ctrl.py checks the rule on
// a machine without a GPU.
#include <hip/hip_runtime.h>

#include "em_trial_seqs.h"
#include "vbhem_em_trial_ctrl.h"

extern "C" {

int trial_ctrl_size() { return (int)sizeof(vbhem::TrialCtrl); }

void trial_ctrl_init(vbhem::TrialCtrl *c) { vbhem::trial_ctrl_init(c); }

int trial_ctrl_step(vbhem::TrialCtrl *c, double L, int max_iter, double minDiff) {
  return vbhem::trial_ctrl_step(c, L, max_iter, minDiff);
}

int emtrialscheck_seq_count() {
  int n = 0;
  emtrialseqs::table(&n);
  return n;
}

// sequence i: its bounds into L [emtrialscheck_seq_max_len()], its settings and hand-made
// outcome; returns the number of bounds, or -1
int emtrialscheck_seq_max_len() { return emtrialseqs::kMaxLen; }

int emtrialscheck_seq(int i, char *name, int name_cap, double *L, int *max_iter, double *minDiff,
                      int *iters, int *stable) {
  int n = 0;
  const emtrialseqs::Seq *s = emtrialseqs::table(&n);
  if (i < 0 || i >= n) return -1;
  int x = 0;
  for (; x + 1 < name_cap && s[i].name[x]; ++x) name[x] = s[i].name[x];
  if (name_cap > 0) name[x] = 0;
  for (int q = 0; q < s[i].n; ++q) L[q] = s[i].L[q];
  *max_iter = s[i].max_iter;
  *minDiff = s[i].minDiff;
  *iters = s[i].iters;
  *stable = s[i].stable;
  return s[i].n;
}

}  // extern "C"
