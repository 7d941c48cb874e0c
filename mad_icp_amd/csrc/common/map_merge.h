// MERGING SAVED ROWS into a voxel map (madicp_map_merge_rows / madicp_host_map_merge_rows) — ONE source for the device kernels
// (csrc/hip/frontend.hip.h: rows_claim / rows_append / rows_combine) and for the host twin (csrc/host/voxel_map.h: merge_rows), so
// they cannot drift apart.  Everything here is integer arithmetic or a copy of bits: no floating-point operation at all.
//
// The rule.  A BATCH is n entries (key_i, xyz_i[3] float32, attr_i, e_i, M_i[10]) — what the window downloads of a map hand out
// (madicp_map_download_rows / _evidence / _moments); attr, e and M are there exactly when the map has that column.  A merge is ONE
// fold of the map: on a moments map it takes the next fold ordinal, and it is refused where a fold of a cloud would be
// (kMomentsLastOrdinal).
//   rows      the keys of the batch that the map does not hold become one new row each, appended in ascending order of the LOWEST
//             index that carries the key; xyz and attr come from that entry, copied bit for bit (NaN payloads and -0.0 stay), the
//             stored key is the entry's key.  Nothing checks that xyz lies in the voxel of its key: a float row cannot reproduce its
//             key (export_point.h).  Rows the map already holds keep their xyz, attr and position.
//   evidence  s = the sum of e_i over the entries of a key, as a wide integer; a new row gets min(s, cap), a row that held e gets
//             min(e + s, cap).  Saturating addition commutes — min(min(e + a, cap) + b, cap) == min(e + a + b, cap) — so the order of
//             arrival decides nothing, and merge_evidence below, one entry at a time, gives it.  What a fold keeps per table slot to
//             hit a row once (the device's stamp and fold count) is not touched: a merge is no hit.
//   moments   voxel_moments.h's own rule with entries in place of points: a row takes ALL entries of its key iff its n BEFORE the
//             merge is < max_count — a new row has n = 0 and takes all — else none; the ten words add; the add that brings n to or
//             past max_count closes the row with the merge's ordinal (moment_row_takes / moment_closes, unchanged: the intervals
//             [old, old + n_i) of a row's entries tile its count, so exactly one add sees old < max_count <= old + n_i).
// Nothing can wrap — voxel_moments.h's argument word for word: the batch's counts sum to at most 2^31 - 1, a row that takes them
// had n < max_count <= 2^31 before, so n < 2^32 always; an entry is refused unless S1[a] <= 65535 n_i and S2 <= 65535^2 n_i, what
// n_i points of 16-bit offsets can reach at most, so S1 < 2^48 and S2 < 2^64 stay true of every row.
// Moments of two maps of the same frame and voxel size therefore ADD exactly: with max_count = 2^31, merging the rows of map(X)
// into map(Y) gives, key by key, the ten words of a map folded from X's and Y's clouds (row order and xyz may differ: who came
// first is not the same question).  Restoring a saved map is merging into an empty one.
// A function of (map, batch) alone: bit-equal between the device, the host twin and a numpy restatement (tests/map_merge_ref.py).
#pragma once
#include <cstdint>

#include "export_point.h"
#include "voxel_moments.h"

namespace madicp_host {

constexpr uint32_t kMergeEvidenceMax = 0x7fffffffu;            // e_i: 1 .. 2^31 - 1 (what a map's word can be: kMapEvidenceCapMax)
constexpr uint64_t kMergeCountMax = 0x7fffffffull;             // the batch's total of n_i, and so every n_i: at most 2^31 - 1
constexpr uint64_t kMergeOffsetMax = 65535ull;                 // a quantised offset (voxel_moments.h: w < 2^16)

// the columns of a batch as the caller gave them (null: not given), and what of the map decides a refusal
struct MergeBatch {
  const uint64_t* keys;
  const float* xyz;      // (n, 3)
  const uint32_t* attr;  // (n)
  const uint32_t* ev;    // (n)
  const uint64_t* mom;   // (n, 10)
  int64_t n;
};
struct MergeTarget {
  double voxel;
  bool with_attr, with_ev, with_mom;
  int64_t rows, max_rows;
  uint32_t ordinal;  // moments maps: the folds since creation or clear
};

// What both entry points refuse, in ONE O(n) pass before anything else — on a refusal the map is untouched (null = nothing to
// refuse).  *capacity: the refusal is MADICP_ERR_CAPACITY's (the fold's conservative rule, decided without looking at a key, and the
// last fold ordinal), else MADICP_ERR_INVALID's.  With n == 0 the columns may be null, and the call does nothing.
inline const char* map_merge_refusal(const MergeBatch& B, double voxel, const MergeTarget& T, bool* capacity) {
  *capacity = false;
  if (B.n < 0 || B.n > kMapMaxRows) return "n: 0 .. 2^30";
  if (!(voxel == T.voxel)) return "voxel: not the map's (moments and keys of another voxel size mean other cells)";
  if ((B.attr && !T.with_attr) || (B.ev && !T.with_ev) || (B.mom && !T.with_mom)) return "a column the map was made without";
  if (B.n > 0 && (!B.keys || !B.xyz || (T.with_attr && !B.attr) || (T.with_ev && !B.ev) || (T.with_mom && !B.mom)))
    return "a column the map has is missing (null)";
  uint64_t total = 0;
  for (int64_t i = 0; i < B.n; ++i) {
    if (B.keys[i] >> 63) return "keys: bit 63 is never set in a voxel key";
    if (T.with_ev && (B.ev[i] < 1 || B.ev[i] > kMergeEvidenceMax)) return "evidence: every word 1 .. 2^31 - 1";
    if (!T.with_mom) continue;
    const uint64_t* M = B.mom + kMomentWords * i;
    if (M[0] < 1) return "moments: every entry's count at least 1";
    if (M[0] > kMergeCountMax) return "moments: the counts of a batch sum to at most 2^31 - 1";
    total += M[0];  // (at most 2^30 entries of less than 2^31: no wrap)
    for (int a = 0; a < 3; ++a)
      if (M[1 + a] > kMergeOffsetMax * M[0]) return "moments: a sum above 65535 times its count";
    for (int a = 0; a < 6; ++a)
      if (M[4 + a] > kMergeOffsetMax * kMergeOffsetMax * M[0]) return "moments: a sum of products above 65535^2 times its count";
  }
  if (total > kMergeCountMax) return "moments: the counts of a batch sum to at most 2^31 - 1";
  *capacity = true;
  if (T.rows + B.n > T.max_rows) return "the map's rows and the batch's entries together exceed max_rows";
  if (T.with_mom && B.n > 0 && T.ordinal > kMomentsLastOrdinal) return "the moments map has folded 2^32 - 1 times since it was made or cleared";
  *capacity = false;
  return nullptr;
}

// the word of a row that held e (0: a row this merge has just made) after one entry's e_i — in 64 bits, e + min(e_i, cap) <= 2 cap
MADICP_HD inline uint32_t merge_evidence(uint32_t e, uint32_t e_i, uint32_t cap) {
  const uint64_t s = static_cast<uint64_t>(e) + (e_i < cap ? e_i : cap);
  return s < cap ? static_cast<uint32_t>(s) : cap;
}

}  // namespace madicp_host
