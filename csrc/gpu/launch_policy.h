// Launch policy of the stream loader (host only, no HIP calls).
//
// Assembled batches wait in the loader's pending list, each already bound to
// a consumer-posted output buffer, until this policy says "flush": then every
// waiting direct-path batch goes out in ONE kernel (loader.cpp:
// flush_pending).  The policy is a pure function of a handful of counts, so
// the decision can be exercised on the CPU (csrc/tests/launch_policy_check.cpp
// runs it inside a discrete-event model of worker, GPU queue and consumer).
//
// Rules, in order:
//   * nothing pending: nothing to do;
//   * end of stream or stop: flush, nothing more will join the batches;
//   * a copy-path batch is pending: flush, such a batch launches alone and at once;
//   * room (fewer than launch_depth launches in flight): flush, the batch
//     starts no later than it could;
//   * one more batch would exceed the launch's image cap: flush;
//   * the worker is out of posted output buffers: flush only while fewer than
//     max(1, launch_depth) launches are in flight.  With that many queued the
//     GPU has work for at least one more kernel time; a batch forced out
//     behind them starts no sooner for it and pays the fixed cost of a launch
//     alone.  Held, it leaves with its neighbours when a launch retires and
//     room opens.  The max(1, ..) keeps launch_depth = 0 alive: with no buffer
//     and nothing in flight nothing would ever retire to free a buffer;
//   * otherwise hold.
#pragma once

namespace btn {
namespace gpu {
namespace policy {

struct State {
  int pending_batches = 0;     // assembled, bound to a buffer, not launched
  int pending_images = 0;
  bool copy_waiting = false;   // one of them takes the copy path
  int inflight = 0;            // launches queued on the GPU and not seen retired
  int launch_depth = 2;        // LoaderConfig::launch_depth
  int batch_size = 1;
  int max_images = 64;         // images one launch can hold (kernels.h: kMaxSrcs)
  bool out_of_buffers = false; // the worker holds a complete batch and no posted buffer to bind it to
  bool ending = false;         // nothing more will join: stream complete, or a caller that drains on stop
};

// `force_floor` is the least number of launches in flight that lets an
// out-of-buffers worker hold; it is 1 everywhere but in the policy's own test,
// which shows that 0 hangs a launch_depth = 0 stream.
inline bool decide(const State& s, int force_floor) {
  if (s.pending_batches <= 0) return false;
  if (s.ending || s.copy_waiting) return true;
  if (s.inflight < s.launch_depth) return true;
  if (s.pending_images + s.batch_size > s.max_images) return true;
  const int hold_at = s.launch_depth > force_floor ? s.launch_depth : force_floor;
  return s.out_of_buffers && s.inflight < hold_at;
}

inline bool flush_now(const State& s) { return decide(s, 1); }

}  // namespace policy
}  // namespace gpu
}  // namespace btn
