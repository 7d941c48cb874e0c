// Registering a scan against the SURFELS of the voxel map (madicp_map_register_cloud / madicp_host_map_register) — ONE source for
// the device kernels (csrc/hip/frontend.hip.h: map_align_terms / map_align_join / map_align_step) and for the host twin
// (csrc/host/voxel_map.h: VoxelMap::align), so they cannot drift apart.  Like export_point.h, every translation unit that includes
// this is compiled WITHOUT floating-point contraction.  fp64 and integers only, no library function in the linearisation.
//
// The rule.  Parameters: reach (0 or 1), max_dist (>= 0, +inf legal), rho (> 0, +inf = no robust kernel), min_count (>= 3), flat
// (in (0, 1]).  The surfel columns — centroid, normal, eig as float32, count as uint32 — are what map_surfel (voxel_moments.h)
// gives for every row.  Point i with cloud-frame position p, at pose (R, t):
//   1  q = export_position(p, R, t); a candidate as export_cells says
//   2  its row j is the QUERY's answer at `reach` (export_point.h: the smallest (d2, j) from the stored float row) — the same rule,
//      not a second one; matched iff j >= 0, within iff also d2 <= max_dist * max_dist
//   3  an inlier iff within, count[j] >= min_count, (double)eig[j][1] > 0 and (double)eig[j][0] <= flat * (double)eig[j][1]
//      (align_inlier).  eig1 > 0 is a statement about the geometry, not about rounding: map_surfel's ZERO RULE (voxel_moments.h)
//      delivers +0.0 for an eigenvalue the solve cannot tell from zero, so identical or collinear points — no plane — are refused,
//      and an exact plane (eig0 == +0.0 < eig1) passes at every flat
//   4  with c, n the float32 centroid and normal of row j taken to double (align_terms):
//        e    = sum3s(n0 (q0 - c0), n1 (q1 - c1), n2 (q2 - c2))
//        m[k] = sum3s(n0 R[k], n1 R[3 + k], n2 R[6 + k])                  n^T R
//        J    = [m, p x m]                                                the reference's [n^T R, -n^T R skew(p)] (mad_icp.cpp:59-103)
//                                                                         for the right-multiplied update X <- X * dX
//        a = fabs(e), s = a > rho ? rho / a : 1.0                         the reference's kernel; rho is its rho_ker_
//        28 terms, sJ[r] = s J[r]:  H(r, c) = sJ[r] J[c] for r >= c at 6c - c(c - 1)/2 + r - c  |  b[r] = sJ[r] e at 21 .. 26  |
//        chi2 = (s e) e at 27                                             — the packing of the round kernels' `total`
//      a point that is no inlier has 28 terms of +0.0
//   5  THE SUM: the n term vectors, padded with +0.0 to the next power of two, are added by the adjacent-pair binary tree in point
//      order, x'[k] = x[2k] + x[2k + 1], level by level: a function of (map, cloud, pose, parameters) alone.  Adding +0.0 changes
//      no value, so a side may run MORE levels than the padding needs (a workgroup always runs eight) — align_tree below is the
//      host's, the shortest form.
//   6  counts: candidates, matched, within, inliers — integers
//   7  a round linearises at X_k and takes X_{k+1} = X_k * dX from dx = H^-1 (-b), dX = (expSO3(dx[3..5]), dx[0..2]); an all-zero H
//      leaves the pose where it is
#pragma once
#include <cmath>
#include <cstdint>

#include "export_point.h"

namespace madicp_host {

constexpr int kAlignTerms = 28;           // H (21, packed lower triangle) | b (6) | chi2
constexpr int kAlignTraceRow = 40;        // X (12: R row-major, t) | the 28 sums
constexpr int kAlignCounts = 4;           // candidates, matched, within, inliers
constexpr int kAlignMaxIterations = 64;
constexpr int kAlignBlock = 256;          // points a device workgroup sums: eight levels of the tree

// the parameters as the C++ layers pass them (madicp_map_align_params of the C ABI, field for field); the defaults are the NEUTRAL
// ones — every matched row with a normal counts, no robust kernel — not tuned ones
struct AlignParams {
  int reach = 1;
  double max_dist = __builtin_huge_val();
  double rho = __builtin_huge_val();
  uint32_t min_count = 3;
  double flat = 1.0;
};

// what both entry points refuse before they look at a point (null = nothing to refuse): the query's conditions and the gates' ranges
inline const char* map_align_refusal(const double* R, const double* t, int reach, double max_dist, double rho, uint32_t min_count,
                                     double flat) {
  if (const char* why = map_query_refusal(R, t, reach, max_dist)) return why;
  if (!(rho > 0.0)) return "rho: > 0 and not NaN (+inf = no robust kernel)";
  if (min_count < 3) return "min_count: at least 3 (a normal needs three points)";
  if (!(flat > 0.0 && flat <= 1.0)) return "flat: in (0, 1]";
  return nullptr;
}

// step 3: `within` is step 2's; count and eig are row j's
MADICP_HD inline bool align_inlier(bool within, uint32_t count, const float* eig, uint32_t min_count, double flat) {
  const double e0 = static_cast<double>(eig[0]), e1 = static_cast<double>(eig[1]);
  return within && count >= min_count && e1 > 0.0 && e0 <= flat * e1;
}

// step 4 for an inlier: the 28 terms into x, the error e returned
MADICP_HD inline double align_terms(const double* p, const double* R, const double* q, const float* centroid, const float* normal,
                                    double rho, double* x) {
  const double n0 = static_cast<double>(normal[0]), n1 = static_cast<double>(normal[1]), n2 = static_cast<double>(normal[2]);
  const double c0 = static_cast<double>(centroid[0]), c1 = static_cast<double>(centroid[1]), c2 = static_cast<double>(centroid[2]);
  const double e = sum3s(n0 * (q[0] - c0), n1 * (q[1] - c1), n2 * (q[2] - c2));
  double J[6];
  for (int k = 0; k < 3; ++k) J[k] = sum3s(n0 * R[k], n1 * R[3 + k], n2 * R[6 + k]);
  J[3] = p[1] * J[2] - p[2] * J[1];
  J[4] = p[2] * J[0] - p[0] * J[2];
  J[5] = p[0] * J[1] - p[1] * J[0];
  const double a = fabs(e);
  const double s = a > rho ? rho / a : 1.0;
  double sJ[6];
  for (int r = 0; r < 6; ++r) sJ[r] = s * J[r];
  int v = 0;
  for (int c = 0; c < 6; ++c)
    for (int r = c; r < 6; ++r) x[v++] = sJ[r] * J[c];
  for (int r = 0; r < 6; ++r) x[21 + r] = sJ[r] * e;
  x[27] = (s * e) * e;
  return e;
}

// step 5 on the host, in place: x holds `rows` vectors of kAlignTerms doubles and ends with the total in its first vector (rows >= 1)
inline void align_tree(double* x, int64_t rows) {
  for (int64_t len = rows; len > 1; len = (len + 1) / 2)
    for (int64_t k = 0; 2 * k < len; ++k) {
      const double* a = x + kAlignTerms * (2 * k);
      double* o = x + kAlignTerms * k;
      if (2 * k + 1 < len)
        for (int c = 0; c < kAlignTerms; ++c) o[c] = a[c] + a[kAlignTerms + c];
      else
        for (int c = 0; c < kAlignTerms; ++c) o[c] = a[c] + 0.0;
    }
}

}  // namespace madicp_host
