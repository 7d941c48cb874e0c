// What happens to ONE point of a registered scan on its way OUT — ONE source for the device export kernels (csrc/hip/frontend.hip.h:
// voxel_claim / voxel_mark / voxel_rows) and for the host twins (csrc/host/cloud_export.h, voxel_map.h), so they cannot drift apart:
// the position in the target frame, the float that goes out, and the voxel a position falls in.  Every translation unit that
// includes this is compiled WITHOUT floating-point contraction (-ffp-contract=off; the device header adds the pragma).
//
// The rule (include/madicp_hip.h: madicp_cloud_export_f32), everything in fp64:
//   position  q[i] = t[i] + (R[3i] p0 + (R[3i+1] p1 + R[3i+2] p2))   — the order of pose * point in the stamped deskew and the
//             sources ingest (sensor_to_base's default branch)
//   output    (float)q[i], round to nearest even; overflow to +-inf as IEEE gives it
//   voxel > 0 cell f = floor(q[i] / voxel) per axis, a true division; the point is a CANDIDATE only if all three satisfy
//             -2^20 <= f < 2^20 (NaN and +-inf fail every comparison: dropped); key = (kx + 2^20) | (ky + 2^20) << 21 |
//             (kz + 2^20) << 42; of the candidates that share a key the one with the LOWEST index is kept, kept points go out in
//             ascending index order
//   voxel == 0 every point goes out, in cloud order, NaN rows included
#pragma once
#include <cmath>
#include <cstdint>

#include "eig3.h"  // MADICP_HD, sum3s

namespace madicp_host {

constexpr double kExportCellMin = -1048576.0, kExportCellEnd = 1048576.0;  // -2^20 <= cell < 2^20
constexpr uint64_t kExportNoKey = ~uint64_t(0);  // "not a candidate"; bit 63 of a real key is never set (3 x 21 bits)

MADICP_HD inline void export_position(const double* p, const double* R, const double* t, double* q) {
  q[0] = t[0] + sum3s(R[0] * p[0], R[1] * p[1], R[2] * p[2]);
  q[1] = t[1] + sum3s(R[3] * p[0], R[4] * p[1], R[5] * p[2]);
  q[2] = t[2] + sum3s(R[6] * p[0], R[7] * p[1], R[8] * p[2]);
}

MADICP_HD inline float export_value(double q) { return static_cast<float>(q); }

// the key of the voxel a position falls in, kExportNoKey when the point is no candidate; voxel > 0
MADICP_HD inline uint64_t export_key(const double* q, double voxel) {
  uint64_t key = 0;
  for (int i = 0; i < 3; ++i) {
    const double f = floor(q[i] / voxel);
    if (!(f >= kExportCellMin && f < kExportCellEnd)) return kExportNoKey;
    key |= static_cast<uint64_t>(static_cast<int64_t>(f) + 1048576) << (21 * i);
  }
  return key;
}

// the same decision with the three cells kept (the map query's neighbourhood starts from them): false when the point is no
// candidate; export_key(q, voxel) == export_key_of_cells(cell) for every candidate (tests/cpp/map_query_check.cpp)
MADICP_HD inline bool export_cells(const double* q, double voxel, int32_t* cell) {
  for (int i = 0; i < 3; ++i) {
    const double f = floor(q[i] / voxel);
    if (!(f >= kExportCellMin && f < kExportCellEnd)) return false;
    cell[i] = static_cast<int32_t>(f);
  }
  return true;
}
MADICP_HD inline uint64_t export_key_of_cells(const int32_t* cell) {  // every cell in [-2^20, 2^20)
  uint64_t key = 0;
  for (int i = 0; i < 3; ++i) key |= static_cast<uint64_t>(static_cast<int64_t>(cell[i]) + 1048576) << (21 * i);
  return key;
}

// what both entry points refuse before they look at a point (null = nothing to refuse)
inline const char* export_refusal(const double* R, const double* t, double voxel) {
  if (!R || !t) return "null argument";
  for (int i = 0; i < 9; ++i)
    if (!(R[i] - R[i] == 0.0)) return "R and t: finite entries";
  for (int i = 0; i < 3; ++i)
    if (!(t[i] - t[i] == 0.0)) return "R and t: finite entries";
  if (!(voxel - voxel == 0.0) || voxel < 0.0) return "voxel: finite and >= 0 (0 = every point)";
  return nullptr;
}

// ---- the voxel map (madicp_map_* / madicp_host_map_*): the same per-point rule, folded into a set of keys that persists ----------
constexpr int64_t kMapMaxRows = int64_t(1) << 30;               // (the device table has two 32-bit-indexed slots per row)

// what both create entry points refuse (null = nothing to refuse): a map has no "every point" mode
inline const char* map_create_refusal(double voxel, int64_t initial_rows, int64_t max_rows) {
  if (!(voxel - voxel == 0.0) || !(voxel > 0.0)) return "voxel: finite and > 0";
  if (initial_rows < 1) return "initial_rows: at least 1";
  if (max_rows < 1 || max_rows > kMapMaxRows) return "max_rows: 1 .. 2^30";
  return nullptr;
}

// ---- pruning the map (madicp_map_prune / madicp_host_map_prune): rows beyond `radius` of `center` leave, with their keys ------------
// what both prune entry points refuse (null = nothing to refuse)
inline const char* map_prune_refusal(const double* center, double radius) {
  if (!center) return "null argument";
  for (int i = 0; i < 3; ++i)
    if (!(center[i] - center[i] == 0.0)) return "center: finite entries";
  if (!(radius - radius == 0.0) || !(radius > 0.0)) return "radius: finite and > 0";
  if (!(radius * radius - radius * radius == 0.0)) return "radius: its square must be finite";
  return nullptr;
}

// whether a row stays: fp64, from the STORED float row (all a map keeps of a position); r2 = radius * radius, computed once by the
// caller.  A distance of exactly `radius` stays; a row that fails the comparison for any reason (a NaN or infinite float) leaves.
MADICP_HD inline bool map_row_kept(const float* row, const double* c, double r2) {
  const double dx = static_cast<double>(row[0]) - c[0];
  const double dy = static_cast<double>(row[1]) - c[1];
  const double dz = static_cast<double>(row[2]) - c[2];
  return sum3s(dx * dx, dy * dy, dz * dz) <= r2;
}

// ---- clearing the map by a scan's rays (madicp_map_clear_rays / madicp_host_map_clear_rays): rows that a ray passes through leave ---
// A ray runs from the sensor origin qo to a point q of the scan, both in the map frame (export_position).  It is SAMPLED one voxel
// edge apart — sample k = 1 .. K sits k * voxel along it — which is not an exact voxel traversal: a ray can cut a voxel's corner
// between two samples.  That is the rule.  Everything fp64, no contraction:
//   d[a] = q[a] - qo[a],  L = sqrt(dx dx + (dy dy + dz dz))
//   K    = min(floor((L - margin) / voxel), kRayMaxSamples) if L is finite and L - margin >= voxel, else 0 (ray_sample_count)
//   s[a] = qo[a] + d[a] * f,  f = (k * voxel) / L — three separate operations per axis (ray_sample)
// The candidate keys of the samples are TRAVERSED (T), the candidate keys of the end points are OCCUPIED by this scan (O); a row
// leaves iff its STORED key is in T \ O.  A sample outside the key range is skipped, the walk goes on behind it.
constexpr int kRayMaxSamples = 4096;  // bounds the work of one ray: the voxels beyond kRayMaxSamples * voxel of the origin stay

// what both entry points refuse (null = nothing to refuse): export_refusal's conditions on R and t, a finite origin and margin >= 0
inline const char* map_clear_refusal(const double* R, const double* t, const double* origin, double margin) {
  if (!R || !t || !origin) return "null argument";
  if (const char* why = export_refusal(R, t, 1.0)) return why;
  for (int i = 0; i < 3; ++i)
    if (!(origin[i] - origin[i] == 0.0)) return "origin: finite entries";
  if (!(margin - margin == 0.0) || margin < 0.0) return "margin: finite and >= 0";
  return nullptr;
}

// d = q - qo and the length of the ray
MADICP_HD inline double ray_length(const double* qo, const double* q, double* d) {
  d[0] = q[0] - qo[0];
  d[1] = q[1] - qo[1];
  d[2] = q[2] - qo[2];
  return sqrt(sum3s(d[0] * d[0], d[1] * d[1], d[2] * d[2]));
}

// samples a ray of length L walks: 0 for a NaN or infinite length and for one below voxel + margin
MADICP_HD inline int ray_sample_count(double L, double margin, double voxel) {
  if (!(L - L == 0.0)) return 0;
  const double reach = L - margin;
  if (!(reach >= voxel)) return 0;
  const double k = floor(reach / voxel);
  return k < static_cast<double>(kRayMaxSamples) ? static_cast<int>(k) : kRayMaxSamples;
}

// sample k (1 .. K) of the ray
MADICP_HD inline void ray_sample(const double* qo, const double* d, double L, int k, double voxel, double* s) {
  const double f = (static_cast<double>(k) * voxel) / L;
  s[0] = qo[0] + d[0] * f;
  s[1] = qo[1] + d[1] * f;
  s[2] = qo[2] + d[2] * f;
}

// ---- evidence (madicp_map_create_ev / madicp_host_map_create_ev): a hit/miss count per row, integers only ---------------------------
// A map made with evidence has three parameters fixed at creation — hit, miss, cap — and one 32-bit word e per row, 1 <= e <= cap:
//   fold      a row the fold creates gets e = hit; a row that was there before it and whose STORED key is a candidate key of the
//             folded cloud gets e = min(e + hit, cap) — once per fold, however many points fall into the voxel
//   clearing  a row whose stored key is in T \ O is MISSED: e > miss -> it stays with e - miss, else it leaves (the prune's close-up,
//             watermark and removal log); the rule covers every row, and the decrements hold even when no row leaves
// hit = miss = cap = 1 is the plain map: every row holds 1, a hit saturates at once, a miss removes.
constexpr uint32_t kMapEvidenceCapMax = 0x7fffffffu;  // e + hit <= 2 cap stays within 32 bits

// what both create entry points refuse (null = nothing to refuse)
inline const char* map_evidence_refusal(uint32_t hit, uint32_t miss, uint32_t cap) {
  if (hit < 1) return "evidence: hit at least 1";
  if (miss < 1) return "evidence: miss at least 1";
  if (cap < hit) return "evidence: cap at least hit";
  if (cap > kMapEvidenceCapMax) return "evidence: cap at most 2^31 - 1";
  return nullptr;
}

// the word of a row after a fold that hit it
MADICP_HD inline uint32_t map_evidence_hit(uint32_t e, uint32_t hit, uint32_t cap) {
  const uint32_t s = e + hit;  // (e <= cap, hit <= cap, cap < 2^31: no wrap)
  return s < cap ? s : cap;
}

// a clearing that missed the row: whether it stays; *e is its word afterwards (unchanged where it leaves)
MADICP_HD inline bool map_evidence_miss(uint32_t* e, uint32_t miss) {
  if (*e <= miss) return false;
  *e -= miss;
  return true;
}

// ---- querying the map (madicp_map_query_cloud / madicp_host_map_query): the nearest row per point, the map only read ---------------
// Point i goes through (R, t) as everywhere (export_position) and, if it is a candidate, has its three cells (export_cells).  Its
// NEIGHBOURHOOD is the cells cell + o, o in {-reach .. reach}^3, reach 0 or 1; a cell with an axis outside [-2^20, 2^20) is skipped
// (nothing wraps).  For every row j whose STORED key is the key of a cell of the neighbourhood the squared distance comes from the
// stored float row — map_row_kept's association, fp64, no contraction (query_d2) — and the answer is the row with the smallest
// (d2, j), lexicographically: a tie goes to the lower row.  A minimum does not depend on the order of its arguments, so the answer
// is a function of (map, cloud, pose, reach) alone.  No candidate, or no such row: row -1, d2 +inf, key kExportNoKey, words 0.  A
// row whose d2 is NaN (a stored NaN float) is never the answer.  Everything is fp64 or integer and calls no library function.
constexpr int kQueryCells = 27;  // the neighbourhood at reach 1; cell c has the offset (c % 3 - 1, c / 3 % 3 - 1, c / 9 - 1)
constexpr int kQueryOwnCell = 13;  // ... whose middle one is the point's own: all there is at reach 0
constexpr double kQueryNoDistance = __builtin_huge_val();  // +inf: the d2 of "no row"

// what both entry points refuse (null = nothing to refuse): export_refusal's conditions on R and t, reach 0 or 1, max_dist >= 0
inline const char* map_query_refusal(const double* R, const double* t, int reach, double max_dist) {
  if (!R || !t) return "null argument";
  if (const char* why = export_refusal(R, t, 1.0)) return why;
  if (reach != 0 && reach != 1) return "reach: 0 or 1";
  if (!(max_dist >= 0.0)) return "max_dist: >= 0 and not NaN (+inf is legal)";
  return nullptr;
}

// the key of cell c (0 .. kQueryCells - 1) of the neighbourhood of `cell`; false where an axis leaves the key range
MADICP_HD inline bool query_cell_key(const int32_t* cell, int c, uint64_t* key) {
  const int32_t o[3] = {c % 3 - 1, c / 3 % 3 - 1, c / 9 - 1};
  int32_t nb[3];
  for (int i = 0; i < 3; ++i) {
    nb[i] = cell[i] + o[i];
    if (nb[i] < -1048576 || nb[i] >= 1048576) return false;
  }
  *key = export_key_of_cells(nb);
  return true;
}

// the squared distance of a position to a stored float row
MADICP_HD inline double query_d2(const double* q, const float* row) {
  const double dx = q[0] - static_cast<double>(row[0]);
  const double dy = q[1] - static_cast<double>(row[1]);
  const double dz = q[2] - static_cast<double>(row[2]);
  return sum3s(dx * dx, dy * dy, dz * dz);
}

// whether (d2, row) comes before (best_d2, best_row); "no row yet" is (+inf, -1), which every real row beats — -1 is the LARGEST
// row in the unsigned comparison — and a NaN d2 beats nothing
MADICP_HD inline bool query_before(double d2, int32_t row, double best_d2, int32_t best_row) {
  return d2 < best_d2 || (d2 == best_d2 && static_cast<uint32_t>(row) < static_cast<uint32_t>(best_row));
}

// ---- scoring many poses (madicp_map_score_poses / madicp_host_map_score): the query's three counts at each of K poses ---------------
// poses is (K, 12) doubles, R row-major then t (the first 12 entries of a row of the registration's trace).  Point i TAKES PART iff
// i % stride == 0; counts[k] = {candidates, matched, within} are the query's counts, above, of the cloud of the points that take
// part at pose k: the same export_position, export_cells, neighbourhood, (d2, row) order and d2 <= max_dist max_dist in fp64.  Sums
// of integers: a function of (map, cloud, poses, reach, max_dist, stride) alone, equal to K scoring queries of the subsampled cloud.
constexpr int64_t kScoreMaxPoses = 4096;
constexpr int kScorePoseDoubles = 12;

MADICP_HD inline bool score_takes_part(int64_t i, int64_t stride) { return i % stride == 0; }

// what both entry points refuse (null = nothing to refuse); one non-finite entry in any pose refuses the whole call
inline const char* map_score_refusal(const double* poses, int64_t n_poses, int reach, double max_dist, int64_t stride) {
  if (!poses) return "null argument";
  if (n_poses < 1 || n_poses > kScoreMaxPoses) return "n_poses: 1 .. 4096";
  for (int64_t i = 0; i < n_poses * kScorePoseDoubles; ++i)
    if (!(poses[i] - poses[i] == 0.0)) return "poses: finite entries";
  if (reach != 0 && reach != 1) return "reach: 0 or 1";
  if (!(max_dist >= 0.0)) return "max_dist: >= 0 and not NaN (+inf is legal)";
  if (stride < 1) return "stride: at least 1";
  return nullptr;
}

}  // namespace madicp_host
