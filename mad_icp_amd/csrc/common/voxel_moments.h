// Per-voxel MOMENTS of the voxel map (madicp_map_create_mom / madicp_host_map_create_mom) — ONE source for the device kernels
// (csrc/hip/frontend.hip.h: map_moments, map_surfels) and for the host twin (csrc/host/voxel_map.h), so they cannot drift apart.  Like
// export_point.h, every translation unit that includes this is compiled WITHOUT floating-point contraction.
//
// The rule.  A candidate point of a fold (export_point.h: q = export_position, f[a] = floor(q[a] / voxel), the cell export_key packs)
// has a QUANTISED OFFSET inside its voxel, 16 bits per axis:
//   u[a] = q[a] / voxel - f[a]       the same division export_key makes; u in [0, 1] — 1.0 where q[a] is negative and so tiny that
//                                    f is -1 and the subtraction rounds to 1 (q = -1e-20: u = 1.0)
//   w[a] = min((uint32)floor(u[a] * 65536.0), 65535)
// A row of a moments map keeps ten unsigned 64-bit words over the candidate points it has TAKEN:
//   n | S1[3] = sum w[a] | S2[6] = sum w[a] w[b], in the order xx, xy, xz, yy, yz, zz
// Which points a row takes: with max_count (1 .. 2^31, fixed at creation), a row takes ALL candidate points of a fold whose key is
// its stored key iff its n BEFORE that fold is < max_count — the point that creates the row is one of them — else none: a row
// freezes at the end of the fold that brings it to or past max_count.  Integer sums commute: the words do not depend on the order
// in which the points of a fold arrive, nor does the decision, which looks at n before the fold only.
// Nothing can wrap: a fold has at most 2^31 - 1 points (kMapMaxRows = 2^30 bounds a cloud), a row that takes a fold had
// n < max_count <= 2^31 before it, so n < 2^32 always; w < 2^16, so S1 < 2^48 and S2 < 2^64 (2^32 x (2^16 - 1)^2 < 2^64).
// Non-candidates (kExportNoKey) contribute nothing.
//
// The SURFEL of a row, all fp64, from the ten words and the stored key only (map_surfel below):
//   cell[a] = ((key >> 21 a) & 0x1fffff) - 2^20,  m[a] = (double)S1[a] / (double)n
//   centroid  c[a] = ((double)cell[a] + (m[a] + 0.5) / 65536.0) * voxel, as float32   (+ 0.5: the middle of a quantisation step)
//   C_ab      = (double)S2_ab / (double)n - m[a] * m[b]
//   eig3_sym(C): w ascending, V
//   zero_at   = kSurfelZeroShare * w[2] + kSurfelZeroFloor * 2^-52 * max(S2_xx, S2_yy, S2_zz) / n
//   eigenvalues in m^2: w[i] <= zero_at ? +0.0 : w[i] * (s * s) with s = voxel / 65536.0, as float32 (a NaN stays a NaN)
//   normal    column 0 of V as float32, sign as the solver leaves it (no part of the contract); (0, 0, 0) for n < 3
// THE ZERO RULE.  An eigenvalue that is not above what the computation can tell from zero is DELIVERED as +0.0, so that what a
// consumer decides from it (map_align.h: eig1 > 0 refuses a voxel without a plane — identical or collinear points) follows the
// geometry and not the sign of rounding noise: the trigonometric roots of eig3_sym carry an error of about sqrt(2^-52) of w[2] next
// to a double root, which is what a line's two zero eigenvalues are, and came out as -6e-11, +6e-11 for one line and 0, 0 for
// another.  The two coefficients are MEASURED (tests/test_host_map_surfels_exact.py, against the exact integer reference of
// tests/surfel_exact_ref.py over its catalogue of degenerate voxels; tests/cpp/map_surfel_check.cpp measures the first again on
// surfel_solve, the solve without the rule, whenever it runs): the solver's error on an eigenvalue
// that is exactly zero is at most 3.73e-9 of w[2] — kSurfelZeroShare = 2^-24 = 5.96e-8 is 16 times that, four times sqrt(2^-52),
// and half a unit in the last place of w[2] as the float32 it is delivered as; the cancellation in S2 / n - m m, which shows
// where the offsets are large and the spread is small (100 000 points within three quantisation steps of the voxel's top corner),
// was at most 0.43 of 2^-52 max(S2_aa / n) — kSurfelZeroFloor = 4 is nine times that.  In metres: at voxel 0.5 a voxel whose points
// spread over 0.1 m is called a line when its second extent is below 0.1 m * sqrt(5.96e-8) = 24 micrometres, three quantisation
// steps.  The eigenvalues stay ascending (the threshold is one number per row), an exact plane keeps eig0 = +0.0 and eig1 > 0.
// Moments and centroid use no library function: bit-equal between host and device.  The eigen-solve goes through atan2 / cos / sin,
// whose device versions may differ from libm's in the last bit (eig3.h): eigenvalues and normals agree to a tolerance, not to the bit.
#pragma once
#include <cmath>
#include <cstdint>

#include "export_point.h"

namespace madicp_host {

constexpr int kMomentWords = 10;                             // n, S1[3], S2[6]
constexpr uint32_t kMomentsMaxCountMax = 0x80000000u;        // 2^31
constexpr uint32_t kMomentsNeverClosed = 0xffffffffu;        // closed_at of a row that still takes points
constexpr uint32_t kMomentsLastOrdinal = 0xfffffffeu;        // the last fold ordinal a map hands out (all ones means "never")
constexpr double kSurfelZeroShare = 5.9604644775390625e-8;   // 2^-24 of w[2]: the zero rule's share (measured, see above)
constexpr double kSurfelZeroFloor = 4.0;                     // ... and its multiple of 2^-52 max(S2_aa / n)

// what both create entry points refuse (null = nothing to refuse)
inline const char* map_moments_refusal(uint32_t max_count) {
  if (max_count < 1) return "moments: max_count at least 1";
  if (max_count > kMomentsMaxCountMax) return "moments: max_count at most 2^31";
  return nullptr;
}

// the quantised in-voxel offset of a CANDIDATE position q (export_key(q, voxel) != kExportNoKey)
MADICP_HD inline void moment_offset(const double* q, double voxel, uint32_t* w) {
  for (int a = 0; a < 3; ++a) {
    const double d = q[a] / voxel;
    const double u = d - floor(d);
    const double x = floor(u * 65536.0);
    w[a] = x >= 65535.0 ? 65535u : static_cast<uint32_t>(x);
  }
}

// the nine sums one point adds beside n: c[0 .. 2] to S1, c[3 .. 8] to S2 (xx, xy, xz, yy, yz, zz)
MADICP_HD inline void moment_terms(const uint32_t* w, uint64_t* c) {
  const uint64_t x = w[0], y = w[1], z = w[2];
  c[0] = x; c[1] = y; c[2] = z;
  c[3] = x * x; c[4] = x * y; c[5] = x * z;
  c[6] = y * y; c[7] = y * z; c[8] = z * z;
}

// Whether a row takes the points of fold `ordinal`, from its closed_at word — the ONE freeze mechanism of both sides: the add
// that takes n to or past max_count (old < max_count <= old + taken) stores the fold's ordinal there; a row is skipped iff the word
// holds an ordinal other than "never" and other than this fold's.  Within a fold the word only ever goes from "never" to this fold's.
MADICP_HD inline bool moment_row_takes(uint32_t closed_at, uint32_t ordinal) {
  return closed_at == kMomentsNeverClosed || closed_at == ordinal;
}
// `taken` points (>= 1) added at once to a row that held old_n: whether this add is the one that reaches max_count
MADICP_HD inline bool moment_closes(uint64_t old_n, uint32_t taken, uint32_t max_count) {
  return old_n < max_count && max_count <= old_n + taken;
}

// The solve behind a surfel, BEFORE the zero rule: from the ten words M and the means m[a] = S1[a] / n, the covariance's eigenvalues
// w (ascending, offset units squared, as eig3_sym leaves them — rounding noise and its sign included) and eigenvectors V; returns
// the zero rule's threshold zero_at for this row.  Apart from map_surfel its caller is tests/cpp/map_surfel_check.cpp, which
// re-measures on it what the rule's two coefficients stand on.
MADICP_HD inline double surfel_solve(const uint64_t* M, const double* m, double* w, double* V) {
  const double n = static_cast<double>(M[0]);
  const double sxx = static_cast<double>(M[4]) / n, syy = static_cast<double>(M[7]) / n, szz = static_cast<double>(M[9]) / n;
  const double xx = sxx - m[0] * m[0], xy = static_cast<double>(M[5]) / n - m[0] * m[1];
  const double xz = static_cast<double>(M[6]) / n - m[0] * m[2], yy = syy - m[1] * m[1];
  const double yz = static_cast<double>(M[8]) / n - m[1] * m[2], zz = szz - m[2] * m[2];
  const double C[9] = {xx, xy, xz, xy, yy, yz, xz, yz, zz};
  eig3_sym(C, w, V);
  const double sxy = sxx > syy ? sxx : syy;
  return kSurfelZeroShare * w[2] + kSurfelZeroFloor * 2.220446049250313e-16 * (sxy > szz ? sxy : szz);
}

// the surfel of a row: M = its ten words (n >= 1), key = its stored key
MADICP_HD inline void map_surfel(const uint64_t* M, uint64_t key, double voxel, float* centroid, float* normal, float* eig, uint32_t* count) {
  const double n = static_cast<double>(M[0]);
  double m[3];
  for (int a = 0; a < 3; ++a) {
    const double cell = static_cast<double>(static_cast<int64_t>((key >> (21 * a)) & 0x1fffffu) - 1048576);
    m[a] = static_cast<double>(M[1 + a]) / n;
    centroid[a] = static_cast<float>((cell + (m[a] + 0.5) / 65536.0) * voxel);
  }
  double w[3], V[9];
  const double zero_at = surfel_solve(M, m, w, V);
  const double s = voxel / 65536.0;
  const double s2 = s * s;
  const bool flat = M[0] < 3;
  for (int i = 0; i < 3; ++i) {
    // the zero rule (above).  Written so that a NaN is NOT taken for a zero: it is delivered as it is, for a consumer to see
    eig[i] = !(w[i] <= zero_at) ? static_cast<float>(w[i] * s2) : 0.0f;
    normal[i] = flat ? 0.0f : static_cast<float>(V[3 * i]);
  }
  *count = static_cast<uint32_t>(M[0]);
}

}  // namespace madicp_host
