// The host's wait for a sequence number that a kernel releases into pinned memory, written down ONCE: poll the number, look at
// the stream that carries the kernel every so often, apply the two time bounds.  madicp_stream_collect,
// madicp_icp_publish_collect and the tree builder's summary wait are its callers (madicp_capi.hip, frontend_capi.inc.h).  No HIP,
// no RCCL in here: plain C++17 over three callables, so that the branches a test may not provoke on a device — a failed stream,
// a lost rank, a bound that runs out — are checked on the CPU by tests/cpp/seq_wait_check.cpp.  Nothing in here formats a
// message or touches a context: the caller decides what an outcome means for its ticket.
#pragma once
#include <stdint.h>

namespace madicp {

// what a stream probe answers; any other value is the stream's error, handed back to the caller as it is
constexpr int kStreamDone = 0;      // everything enqueued has executed
constexpr int kStreamRunning = -1;

struct WaitLimits {
  int wait_mode = 0;        // option "wait_mode": 0 spin (a probe every 1024th poll), 1 yield / 2 sleep (every 16th)
  int wait_timeout_ms = 0;  // the caller's bound; 0: unbounded
  int comm_timeout_ms = 0;  // the communicator's bound; 0: no communicator
  bool bounded() const { return wait_timeout_ms > 0 || comm_timeout_ms > 0; }
};

enum class WaitOutcome {
  Published,       // *seq == want: everything released before it is visible
  FinishedSilent,  // the stream drained and the number never came
  StreamError,     // the probe reported an error (SeqWait::stream_error)
  CommTimeout,     // comm_timeout_ms ran out and the number is not there: the caller aborts its communicator
  WaitTimeout,     // wait_timeout_ms ran out: the work is still in flight, the same wait may be made again
};
struct SeqWait {
  WaitOutcome outcome;
  int stream_error;  // StreamError only
};

// Waits until *seq == want.  probe() -> kStreamDone / kStreamRunning / an error value; now_ms() -> a millisecond clock;
// pause() -> one poll's pause.  start_ms is the clock's reading the bounds count from — the caller's, so that the waits for
// the scans of one batch share one.
//  - the number is read (acquire) before every pause: once it matches, no probe is made
//  - a drained stream or a communicator over its bound reads the number once more before it gives up: results that are there
//    are never thrown away
//  - the clock is read at a probe only, and only when a bound exists; the communicator's bound goes first
template <class Probe, class Clock, class Pause>
inline SeqWait seq_wait(const int32_t* seq, int32_t want, const WaitLimits& lim, long long start_ms, Probe&& probe, Clock&& now_ms,
                        Pause&& pause) {
  const auto there = [&] { return __atomic_load_n(seq, __ATOMIC_ACQUIRE) == want; };
  const unsigned probe_mask = lim.wait_mode == 0 ? 0x3ffu : 0xfu;  // stream health: every few tens of microseconds
  const bool bounded = lim.bounded();
  for (unsigned polls = 1; !there(); ++polls) {
    if ((polls & probe_mask) == 0) {
      const int q = probe();
      if (q == kStreamDone) return {there() ? WaitOutcome::Published : WaitOutcome::FinishedSilent, 0};
      if (q != kStreamRunning) return {WaitOutcome::StreamError, q};
      if (bounded) {
        const long long ms = now_ms() - start_ms;
        if (lim.comm_timeout_ms > 0 && ms > lim.comm_timeout_ms)
          return {there() ? WaitOutcome::Published : WaitOutcome::CommTimeout, 0};
        if (lim.wait_timeout_ms > 0 && ms > lim.wait_timeout_ms) return {WaitOutcome::WaitTimeout, 0};
      }
    }
    pause();
  }
  return {WaitOutcome::Published, 0};
}

}  // namespace madicp
