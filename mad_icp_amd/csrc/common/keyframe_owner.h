// The ownership rule of the sharded keyframe map, once, for C++ (mad_icp_amd/sharded.py: keyframe_owner is the same
// function; tests/test_shard_pipeline_host.py holds the two to each other).
//
// `k` is the keyframe's ORDINAL in promotion order — the first scan is 0, every promotion adds 1 — not the frame id
// (pipeline.cpp:253 `seq_keyframe_`), which has gaps and would deal unevenly.  The ordinals are dealt in rows of `world`,
// alternate rows in opposite directions: a function of the ordinal alone, so a keyframe never changes hands while the window
// slides, and every window of 2 * world consecutive ordinals gives each rank exactly two trees (num_keyframes = 16 over eight
// ranks: two per rank at every frame).  Alternating rows pair the newest keyframe of one row with the oldest of the next —
// along a trajectory the newest keyframes are the dear ones.
#pragma once
#include <cstdint>

namespace madicp {

// the rank that owns keyframe ordinal k; -1 on bad arguments (k < 0, world < 1)
inline int keyframe_owner(int64_t k, int world) {
  if (k < 0 || world < 1) return -1;
  const int64_t row = k / world;
  const int col = static_cast<int>(k % world);
  return (row % 2 == 0) ? col : world - 1 - col;
}

}  // namespace madicp
