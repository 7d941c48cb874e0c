// KeyframeLedger — the bookkeeping of the (possibly sharded) keyframe window, without a device: which ordinals are in the
// window, which of them this rank owns, which one an eviction takes.  Pipeline pushes and pops its keyframe deque by what
// promote() answers, so the rule that tests/test_shard_pipeline_host.py drives through the host C ABI
// (madicp_host_debug_ledger_*) is the rule the product runs.
//
// The window is GLOBAL: every rank of a sharded Pipeline sees the same scans and takes the same promotion decisions, so every
// rank's ledger goes through the same sequence of ordinals; only `local` differs — keyframe_owner(ordinal, world) == rank.
#pragma once
#include <cstddef>
#include <cstdint>
#include <deque>

#include "../common/keyframe_owner.h"

namespace madicp_host {

class KeyframeLedger {
 public:
  struct Entry {
    int64_t ordinal;
    bool local;  // this rank holds the keyframe's tree
  };
  struct Step {
    Entry promoted;
    bool evicted;      // the window was full: its oldest entry left
    Entry evicted_entry;
  };

  // rank / world as validated by the caller (0 <= rank < world); capacity: Pipeline's num_keyframes
  void configure(int rank, int world, int capacity) {
    rank_ = rank;
    world_ = world;
    capacity_ = capacity;
  }

  // pipeline.cpp:252-257: push the new keyframe, pop the oldest one when the window overflows
  Step promote() {
    Step s{};
    s.promoted = Entry{next_++, true};
    s.promoted.local = madicp::keyframe_owner(s.promoted.ordinal, world_) == rank_;
    window_.push_back(s.promoted);
    n_local_ += s.promoted.local ? 1 : 0;
    s.evicted = window_.size() > static_cast<size_t>(capacity_);  // (the reference's comparison, cast included)
    if (s.evicted) {
      s.evicted_entry = window_.front();
      window_.pop_front();
      n_local_ -= s.evicted_entry.local ? 1 : 0;
    }
    return s;
  }

  int rank() const { return rank_; }
  int world() const { return world_; }
  size_t size() const { return window_.size(); }
  size_t numLocal() const { return n_local_; }
  int64_t promotions() const { return next_; }
  const std::deque<Entry>& window() const { return window_; }

 private:
  int rank_ = 0, world_ = 1, capacity_ = 0;
  int64_t next_ = 0;
  size_t n_local_ = 0;
  std::deque<Entry> window_;
};

}  // namespace madicp_host
