// CPU check of mad_icp_amd/csrc/common/seq_wait.h — the host's wait for a sequence number that a kernel publishes — with a
// scripted stream probe, a fake clock and a counting pause: the outcome of every branch, and exactly how many probes, clock
// reads and pauses it took.  The branches behind a failed stream, a lost rank or a bound that runs out cannot be provoked on a
// device, so this is where they run.  Test infrastructure; compiled and run by tests/test_seq_wait.py (also under ASan + UBSan).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "seq_wait.h"

using namespace madicp;

namespace {

constexpr int32_t kWant = 7;
constexpr int kErr = 719;  // some stream error value: anything but kStreamDone / kStreamRunning

// The world the wait runs in.  The number appears at a scripted moment: behind the n-th pause (the kernel finished while the
// host was polling), during the n-th probe or the n-th clock read (it landed between the poll and the re-read).
struct World {
  int32_t seq = 0;
  long arrive_at_pause = -1, arrive_at_probe = -1, arrive_at_clock = -1;
  std::vector<int> answers;      // probe k answers answers[k - 1]; beyond the script: kStreamRunning
  long long clock_ms = 0;        // the fake clock: every probe takes ms_per_probe
  long long ms_per_probe = 0;
  long probes = 0, clock_reads = 0, pauses = 0;

  SeqWait wait(const WaitLimits& lim, long long start_ms) {
    return seq_wait(
        &seq, kWant, lim, start_ms,
        [this] {
          ++probes;
          clock_ms += ms_per_probe;
          if (probes == arrive_at_probe) seq = kWant;
          return (size_t)probes <= answers.size() ? answers[probes - 1] : kStreamRunning;
        },
        [this] {
          if (++clock_reads == arrive_at_clock) seq = kWant;
          return clock_ms;
        },
        [this] {
          if (++pauses == arrive_at_pause) seq = kWant;
        });
  }
};

int g_cases = 0, g_failed = 0;

void expect(const char* what, int mode, const World& w, const SeqWait& got, WaitOutcome outcome, long probes, long clock_reads, long pauses,
            int stream_error = 0) {
  ++g_cases;
  if (got.outcome == outcome && got.stream_error == stream_error && w.probes == probes && w.clock_reads == clock_reads && w.pauses == pauses)
    return;
  ++g_failed;
  std::printf("FAILED %s (wait_mode %d): outcome %d (want %d), error %d (want %d), probes %ld (want %ld), clock reads %ld (want %ld), "
              "pauses %ld (want %ld)\n",
              what, mode, (int)got.outcome, (int)outcome, got.stream_error, stream_error, w.probes, probes, w.clock_reads, clock_reads,
              w.pauses, pauses);
}

}  // namespace

int main() {
  for (int mode = 0; mode < 3; ++mode) {
    const long c = mode == 0 ? 1024 : 16;  // a probe every c-th poll: modes 1 and 2 share 16
    const WaitLimits unbounded{mode, 0, 0};
    {  // the number is already there: nothing is probed, nothing paused
      World w;
      w.seq = kWant;
      expect("already there", mode, w, w.wait(WaitLimits{mode, 100, 100}, 0), WaitOutcome::Published, 0, 0, 0);
    }
    // the number arrives behind the n-th pause: n pauses, a probe at every c-th poll before it, no clock without a bound ...
    for (long n : {1L, c - 1, c, c + 1, 2 * c + 5, 5 * c}) {
      World w;
      w.arrive_at_pause = n;
      w.ms_per_probe = 1000;  // (however long it takes)
      expect("arrives after n polls, no bound", mode, w, w.wait(unbounded, 0), WaitOutcome::Published, n / c, 0, n);
    }
    // ... and one clock read per probe with either bound set
    for (const WaitLimits& lim : {WaitLimits{mode, 1000, 0}, WaitLimits{mode, 0, 1000}, WaitLimits{mode, 1000, 1000}})
      for (long n : {c - 1, 2 * c + 5}) {
        World w;
        w.arrive_at_pause = n;
        w.ms_per_probe = 1;
        expect("arrives after n polls, bounded", mode, w, w.wait(lim, 0), WaitOutcome::Published, n / c, n / c, n);
      }
    {  // the stream drains at the second probe and the number landed just before: read again, Published
      World w;
      w.answers = {kStreamRunning, kStreamDone};
      w.arrive_at_probe = 2;
      expect("done, there on the re-read", mode, w, w.wait(unbounded, 0), WaitOutcome::Published, 2, 0, 2 * c - 1);
    }
    {  // the stream drains and the number never came (bounded: the clock was read at the first probe only)
      World w;
      w.answers = {kStreamRunning, kStreamDone};
      w.ms_per_probe = 1;
      expect("done, absent", mode, w, w.wait(WaitLimits{mode, 1000, 1000}, 0), WaitOutcome::FinishedSilent, 2, 1, 2 * c - 1);
    }
    {  // the stream reports an error: handed back as it is, before any clock read
      World w;
      w.answers = {kErr};
      w.ms_per_probe = 5000;
      expect("stream error", mode, w, w.wait(WaitLimits{mode, 1000, 1000}, 0), WaitOutcome::StreamError, 1, 0, c - 1, kErr);
    }
    {  // the communicator's bound runs out at the second probe, the number lands during that clock read: results are kept
      World w;
      w.ms_per_probe = 60;
      w.arrive_at_clock = 2;
      expect("comm bound, there on the re-read", mode, w, w.wait(WaitLimits{mode, 0, 100}, 0), WaitOutcome::Published, 2, 2, 2 * c - 1);
    }
    {  // ... and without it: CommTimeout
      World w;
      w.ms_per_probe = 60;
      expect("comm bound, absent", mode, w, w.wait(WaitLimits{mode, 0, 100}, 0), WaitOutcome::CommTimeout, 2, 2, 2 * c - 1);
    }
    {  // exactly the bound is not over it (50, 100, then 150 > 100); only the caller's bound: WaitTimeout, the number untouched ...
      World w;
      w.ms_per_probe = 50;
      expect("wait bound", mode, w, w.wait(WaitLimits{mode, 100, 0}, 0), WaitOutcome::WaitTimeout, 3, 3, 3 * c - 1);
      // ... and the same wait again, from a fresh start, completes
      w.arrive_at_pause = w.pauses + c + 2;
      expect("wait bound, collected again", mode, w, w.wait(WaitLimits{mode, 100, 0}, w.clock_ms), WaitOutcome::Published, 4, 4, 4 * c + 1);
    }
    {  // both bounds over at the same probe: the communicator's goes first
      World w;
      w.ms_per_probe = 200;
      expect("both bounds", mode, w, w.wait(WaitLimits{mode, 50, 110}, 0), WaitOutcome::CommTimeout, 1, 1, c - 1);
    }
    {  // the caller's bound alone is over, the communicator's is not yet: WaitTimeout
      World w;
      w.ms_per_probe = 200;
      expect("wait bound before comm bound", mode, w, w.wait(WaitLimits{mode, 50, 1000}, 0), WaitOutcome::WaitTimeout, 1, 1, c - 1);
    }
    {  // no bound: the clock is never read, however many probes go by, and a clock far ahead times nothing out
      World w;
      w.ms_per_probe = 1 << 20;
      w.arrive_at_pause = 40 * c + 3;
      expect("no bound", mode, w, w.wait(unbounded, 0), WaitOutcome::Published, 40, 0, 40 * c + 3);
    }
    {  // a batch: two waits count from ONE start.  The first takes 60 of the 100 ms; the second is over the bound at its second
       // probe (90, 120) — from a start of its own it would have had two more
      World w;
      w.ms_per_probe = 30;
      w.arrive_at_pause = 2 * c + 3;
      const WaitLimits lim{mode, 100, 0};
      expect("shared start, first scan", mode, w, w.wait(lim, 0), WaitOutcome::Published, 2, 2, 2 * c + 3);
      w.seq = 0;  // (the second scan's number)
      w.arrive_at_pause = -1;
      expect("shared start, second scan", mode, w, w.wait(lim, 0), WaitOutcome::WaitTimeout, 4, 4, 4 * c + 2);
    }
  }
  if (g_failed) {
    std::printf("%d of %d cases FAILED\n", g_failed, g_cases);
    return 1;
  }
  std::printf("seq wait ok: %d cases\n", g_cases);
  return 0;
}
