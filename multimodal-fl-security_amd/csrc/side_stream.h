// A per-device side stream and its events, for the native trainers' overlap of
// one local step's optimizer update (HBM-bound) with the next step's forward
// (MFMA / latency-bound): the update runs on the side stream parameter group
// by parameter group, each group's event recorded after it, and the forward
// waits on a group's event before its first use of those parameters.  Every
// side-stream branch is joined back into the caller's stream within the same
// call, so the entry points stay stream-ordered and capturable in a HIP graph
// (fork / join through events is how a capture spans two streams).
//
// The stream and events are created once per device, outside any capture
// (flr_*_workspace queries create them; a call that finds none while its
// stream is capturing runs the update on the caller's stream instead — same
// results, no overlap).
//
// One stream and one event set per device, shared by every trainer of the
// process: with FLR_SGD_OVERLAP=1 at most one training call may be in flight
// per device at a time (two concurrent callers would record and wait on the
// same events).  A model with more parameter groups than the stream has events,
// less one, updates on the caller's stream (no overlap, same results).
//
// Off by default (FLR_SGD_OVERLAP=1 turns it on).  Measured at C3 on MI355X
// (tools/gpu_r3_k.sh, gpu_r3_l.sh): 79 % of the optimizer's kernel time does
// run concurrently with the forward's kernels, but both slow down by as much
// (summed kernel time 59.3 -> 69.1 ms per round) and the round time is
// unchanged (61.6 vs 61.8-62.2 ms); a side stream created with a priority
// (either end of the range) made the round 50 % slower.
#pragma once

#include <cstdlib>
#include <mutex>

#include "flr_common.h"

namespace flr {

// The native trainers' three auxiliary streams.  Each is one stream and its
// events per device, shared by every trainer of the process (one training call
// per device at a time), created outside any capture and joined back into the
// caller's stream within the call that forks to it.
//
// AUX_OPT: the optimizer's side stream described above.  FLR_SGD_OVERLAP=1
// turns it on, and only in the tools build (FLR_ABLATION): it measured no
// faster.
//
// AUX_TEXT: the text-branch stream of the ResNet + GRU trainer
// (train_clients.hip).  The embedding + GRU forward and backward run on it
// beside the image trunk (the recurrence is a chain of small latency-bound
// launches that leaves most of the chip idle); the trunk's last weight
// gradients follow on it, idle by then.  FLR_TEXT_STREAM=0: everything on the
// caller's stream (A/B).
//
// AUX_WGRAD: the weight-gradient stream.  Every tap-major conv's weight
// gradient (ResNet + GRU) and every ViT layer's weight / bias gradients
// (ViT + BERT) run on it, forked after the layer's output gradient is ready,
// while the caller's stream continues down the data-gradient chain (the
// backward's critical path); joined before the clip + SGD step.  The ResNet's
// forward runs its shortcut convs there.  FLR_WGRAD_STREAM=0: off (A/B).
//
// The gates are read per call.  The event counts decide when a trainer falls
// back to the caller's stream (more parameter groups, layers or forks than
// events: same results, no overlap).
enum AuxKind { AUX_OPT = 0, AUX_TEXT = 1, AUX_WGRAD = 2, AUX_KINDS = 3 };
constexpr int kAuxEvents[AUX_KINDS] = {48, 8, 128};
constexpr int kAuxMaxEvents = 128;

struct AuxStream {
  hipStream_t s = nullptr;
  int nev = 0;  // events created; a stream is handed out only with its kind's full count
  hipEvent_t ev[kAuxMaxEvents] = {};
};

inline bool aux_enabled(AuxKind kind) {
  if (kind == AUX_OPT) {
#ifdef FLR_ABLATION
    return flr::knob_on("FLR_SGD_OVERLAP");
#else
    return false;
#endif
  }
  return !flr::knob_off(kind == AUX_TEXT ? "FLR_TEXT_STREAM" : "FLR_WGRAD_STREAM");
}

// The current device's stream of one kind; created on first use when create is
// set (never during a capture of `st`).  nullptr: none, or the kind is off.
// A creation that fails part-way keeps what it made in the pool, and the next
// creating call completes that set: nothing is leaked or made twice.
inline AuxStream* aux_stream(AuxKind kind, bool create, hipStream_t st = nullptr) {
  if (!aux_enabled(kind)) return nullptr;
  static AuxStream pool[AUX_KINDS][64];
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  AuxStream& a = pool[kind][dev];
  if (a.s && a.nev == kAuxEvents[kind]) return &a;
  if (!create) return nullptr;
  if (st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
  }
  if (!a.s && hipStreamCreateWithFlags(&a.s, hipStreamNonBlocking) != hipSuccess) {
    a.s = nullptr;
    return nullptr;
  }
  for (; a.nev < kAuxEvents[kind]; ++a.nev)
    if (hipEventCreateWithFlags(&a.ev[a.nev], hipEventDisableTiming) != hipSuccess) return nullptr;
  return &a;
}

inline AuxStream* side_stream(bool create, hipStream_t st = nullptr) { return aux_stream(AUX_OPT, create, st); }
inline AuxStream* text_stream(bool create, hipStream_t st = nullptr) { return aux_stream(AUX_TEXT, create, st); }
inline AuxStream* wgrad_stream(bool create, hipStream_t st = nullptr) { return aux_stream(AUX_WGRAD, create, st); }

// Event links between streams (what a capture turns into the graph's edges).
// Each returns an FLR_* status, the failure reported under the call site's label.
inline int ev_record(hipEvent_t e, hipStream_t on, const char* where) {
  return hipEventRecord(e, on) == hipSuccess ? FLR_OK : launch_status(where);
}
inline int ev_wait(hipStream_t s, hipEvent_t e, const char* where) {
  return hipStreamWaitEvent(s, e, 0) == hipSuccess ? FLR_OK : launch_status(where);
}
// e recorded on `from`, then `to` waits on it: a fork, or a join made on the spot
inline int ev_link(hipEvent_t e, hipStream_t from, hipStream_t to, const char* where) {
  if (hipEventRecord(e, from) != hipSuccess || hipStreamWaitEvent(to, e, 0) != hipSuccess) return launch_status(where);
  return FLR_OK;
}

// The next free event of a stream within one step or pass.  left(n): n more can
// be taken (false without a stream).
struct EventCursor {
  AuxStream* a = nullptr;
  int next = 0;
  bool left(int n) const { return a && next + n <= a->nev; }
  hipEvent_t take() { return a->ev[next++]; }
};

}  // namespace flr
