// vbhem_timing.hip -- optional kernel timing of libvbhem_estep.so (bench/profiling):
// hipEvents recorded on the launch stream around each kernel launch; read back (and
// synchronised) only by vbhem_timing_read*.  Off by default.  Per host thread
// (thread_local), like the schedule: the library keeps no state shared between
// threads, so several host threads may drive it at once (the reference MEX is
// re-entrant).  Never recorded into a stream that is being captured into a graph: a
// captured event would be destroyed by the next vbhem_timing_read while the graph
// still records into it on every replay.
// Levels: 1 every timed launch (fb, emission, statistics, gated forward), 2 the fb
// launches only -- two events per E-step, so the instrumentation costs the timed
// region next to nothing (each recorded event is a marker packet the queue
// processes between kernels; a dozen per step was ~40 us at N = 12,500).  Events
// are recycled through a per-thread pool (no create/destroy per launch).
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "vbhem_estep.h"
#include "vbhem_internal.h"

namespace {

struct TimingState {
  int level = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> spans[vbhem::kTimeEmMath + 1];  // by TimingSpan
  std::vector<long long> fb_pairs;
  std::vector<hipEvent_t> pool;
  ~TimingState() {
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
  }
};
thread_local TimingState g_timing;

// timing is recorded for this launch: enabled on this thread and the stream
// is not capturing
bool timing_on(hipStream_t st, bool fb_launch) {
  if (g_timing.level == 0 || (g_timing.level == 2 && !fb_launch)) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return false;
  return cs == hipStreamCaptureStatusNone;
}

// a timing event from the pool, recorded on st or not
hipEvent_t timing_event(hipStream_t st, bool record = true) {
  hipEvent_t ev = nullptr;
  if (!g_timing.pool.empty()) {
    ev = g_timing.pool.back();
    g_timing.pool.pop_back();
  } else if (hipEventCreateWithFlags(&ev, hipEventDisableSystemFence) != hipSuccess) {
    // timing-only events: no system-scope release (an L2 writeback + invalidate
    // per record, ~6 us of idle GPU around each timed kernel at N = 12,500)
    return nullptr;
  }
  if (record) (void)hipEventRecord(ev, st);
  return ev;
}
void timing_recycle(hipEvent_t ev) {
  if (ev) g_timing.pool.push_back(ev);
}

// the spans of one kind: their summed time and count; synchronises, empties the list
int drain(vbhem::TimingSpan span, double *ms_out, long long *n_out, const char *where) {
  auto &v = g_timing.spans[span];
  double t = 0.0;
  int rc = VBHEM_OK;
  const long long n = (long long)v.size();
  for (auto &pr : v) {
    float ms = 0.f;
    if (pr.first && pr.second) {
      hipError_t e = hipEventSynchronize(pr.second);
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, pr.first, pr.second);
      if (e != hipSuccess) rc = vbhem::hip_fail(e, where);
      t += ms;
    }
    timing_recycle(pr.first);
    timing_recycle(pr.second);
  }
  v.clear();
  if (ms_out) *ms_out = t;
  if (n_out) *n_out = n;
  return rc;
}

}  // namespace

namespace vbhem {

hipEvent_t timing_start(hipStream_t st, bool fb_launch, hipEvent_t *end) {
  if (!timing_on(st, fb_launch)) return nullptr;
  if (end && !(*end = timing_event(st, false))) return nullptr;  // both or none
  return timing_event(st, !end);
}
void timing_stop(TimingSpan span, hipEvent_t ev0, hipStream_t st, hipEvent_t ev1, long long fb_pairs) {
  if (!ev0) return;
  g_timing.spans[span].emplace_back(ev0, ev1 ? ev1 : timing_event(st));
  if (span == kTimeFb) g_timing.fb_pairs.push_back(fb_pairs);
}
// EM-loop math kernel timing (vbhem_em.hip), same events and levels as the E-step's
void *timing_begin(hipStream_t st) { return timing_start(st); }
void timing_end_em_math(void *ev0, hipStream_t st) {
  timing_stop(kTimeEmMath, static_cast<hipEvent_t>(ev0), st);
}

}  // namespace vbhem

extern "C" {

int vbhem_timing_enable(int on) {
  g_timing.level = (on == 1 || on == 2) ? on : 0;
  return VBHEM_OK;
}

int vbhem_timing_read(double *fb_ms, long long *fb_launches, long long *fb_pairs, double *stats_ms,
                      long long *stats_launches) {
  int rc = drain(vbhem::kTimeFb, fb_ms, fb_launches, "vbhem_timing_read");
  const int rc_stats = drain(vbhem::kTimeStats, stats_ms, stats_launches, "vbhem_timing_read");
  if (rc_stats != VBHEM_OK) rc = rc_stats;
  long long np = 0;
  for (long long x : g_timing.fb_pairs) np += x;
  g_timing.fb_pairs.clear();
  if (fb_pairs) *fb_pairs = np;
  return rc;
}

int vbhem_timing_read_em_math(double *ms, long long *launches) {
  return drain(vbhem::kTimeEmMath, ms, launches, "vbhem_timing_read_em_math");
}

int vbhem_timing_read_gated(double *fwd_ms, long long *fwd_launches) {
  return drain(vbhem::kTimeGatedForward, fwd_ms, fwd_launches, "vbhem_timing_read_gated");
}

int vbhem_timing_read_emission(double *em_ms, long long *em_launches) {
  return drain(vbhem::kTimeEmission, em_ms, em_launches, "vbhem_timing_read_emission");
}

}  // extern "C"
