// Host side of the conv kernel families (conv.hip, conv_bf16.hip): the one place
// that times candidates, and the one shape-choice path of a launch.
#pragma once
#include <stdlib.h>

#include "conv_common.h"

namespace {
constexpr int kTuneReps = 3;  // launches per timed run

// LD_CONV_TUNE_LOG: 1 = a line per tuned geometry; 2 = the weight gradient's
// candidates too (the conv tuners print at level 1 only)
inline int tune_log_level() {
  const char* lg = getenv("LD_CONV_TUNE_LOG");
  return lg && (lg[0] == '1' || lg[0] == '2') ? lg[0] - '0' : 0;
}

inline double tune_tflops(double flop, float best_ms) {
  return best_ms > 0 ? flop / (best_ms * 1e-3 / kTuneReps) / 1e12 : 0.0;
}

// 1: the geometry is in the table already; LD_EUNSUPPORTED: the stream is
// capturing (timing synchronises); 0: go on and time.
inline int tune_refused(const LdTuneKey& key, hipStream_t stream) {
  LdTuneCfg have;
  if (ld_tune_lookup(key, &have)) return 1;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(stream, &cap);
  return cap != hipStreamCaptureStatusNone ? LD_EUNSUPPORTED : 0;
}

// One timing session.  Quiesces the device first: work queued on other streams
// (the teacher's forward) would share the CUs with some candidates and not others.
class TuneTimer {
 public:
  static constexpr float kLaunchFailed = -2.0f;  // the warm launch returned an error

  explicit TuneTimer(hipStream_t stream) : stream_(stream) {
    (void)hipDeviceSynchronize();
    (void)hipEventCreate(&e0_);
    (void)hipEventCreate(&e1_);
  }
  ~TuneTimer() {
    (void)hipEventDestroy(e0_);
    (void)hipEventDestroy(e1_);
  }

  // ms of kTuneReps launches after a warm one, best of two runs (clocks wander);
  // negative: kLaunchFailed, or -1 when the measurement itself failed
  template <class Launch>
  float time(Launch&& launch) {
    if (launch() != 0) return kLaunchFailed;
    float ms = -1.0f;
    for (int trial = 0; trial < 2; ++trial) {
      (void)hipEventRecord(e0_, stream_);
      for (int rep = 0; rep < kTuneReps; ++rep) launch();
      (void)hipEventRecord(e1_, stream_);
      if (hipEventSynchronize(e1_) != hipSuccess) break;
      float t = 0.0f;
      (void)hipEventElapsedTime(&t, e0_, e1_);
      if (ms < 0.0f || t < ms) ms = t;
    }
    return ms;
  }

 private:
  hipStream_t stream_;
  hipEvent_t e0_, e1_;
};

// Row of a shape table that the record t names, -1 if none.  rec(row) is what the
// family's tuner stores for that row; cap counts only where it holds a shape field.
template <class Cfg, int N, class Rec>
int tune_cfg_index(const Cfg (&tab)[N], const LdTuneCfg& t, Rec rec, bool cap_is_shape) {
  for (int i = 0; i < N; ++i) {
    const LdTuneCfg r = rec(tab[i]);
    if (r.tm == t.tm && r.tn == t.tn && r.wvm == t.wvm && r.d == t.d && r.ks == t.ks &&
        (!cap_is_shape || r.cap == t.cap))
      return i;
  }
  return -1;
}

// The shape of one launch: forced(&rc) first (the family's environment override;
// true = it settled the launch with rc), else the table's record if its row still
// fits, else the model -- a pure function of the geometry.  Never times anything
// and never synchronises.  launch(row, cap): the record's cap, 0 for a model pick.
template <class Cfg, int N, class Forced, class Rec, class Fits, class Model, class Launch>
int launch_picked(int mode, int family, const ConvK& k, const Cfg (&tab)[N], Forced forced,
                  Rec rec, Fits fits, Model model, Launch launch) {
  int rc = 0;
  if (forced(&rc)) return rc;
  int pick = -1;
  LdTuneCfg t;
  if (ld_tune_lookup(make_tune_key(mode, family, k), &t)) {
    pick = tune_cfg_index(tab, t, rec, family == 2);  // C8: cap is the schedule
    if (pick >= 0 && !fits(k, tab[pick])) pick = -1;
  }
  const int cap = pick >= 0 ? t.cap : 0;
  if (pick < 0) pick = model(k);
  if (pick < 0) return LD_EUNSUPPORTED;
  return launch(tab[pick], cap);
}
}  // namespace
