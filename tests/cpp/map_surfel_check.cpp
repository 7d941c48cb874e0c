// Stand-alone check of the voxel map's surfel and of the gate that stands on it (csrc/common/voxel_moments.h: map_surfel over
// csrc/common/eig3.h: eig3_sym; csrc/common/map_align.h: align_inlier) under AddressSanitizer and UndefinedBehaviorSanitizer: compiled
// and run by tests/test_map_surfel_sanitized.py.  The populations are those of tests/surfel_exact_ref.py's catalogue, built here from
// integers: identical points, lines along an axis, a face diagonal and (5, 3, 1), exact planes, a square, a cube, a tetrahedron,
// populations of one to four, 100 000 points at the voxel's top corner — each at the bottom, the middle and the top of the voxel,
// under the six axis permutations and the reflection w -> 65535 - w.  The ten words live in a heap block of EXACTLY ten, the outputs in
// blocks of EXACTLY three floats.  What is held: everything finite, eigenvalues ascending and never negative (the zero rule), the
// normal of unit length or (0, 0, 0) below three points, and the decision by KIND — points and lines are never inliers, exact planes
// and solids with at least min_count points always at flat = 1.
// It also MEASURES, on surfel_solve — the solve without the zero rule — what the rule's share stands on: over the points and lines,
// whose eigenvalues 0 and 1 are exactly zero, the worst |w_i| as a share of w2 (3.73e-9 when the rule was set), in floors where the
// floor carries it, and as a share of the rule's threshold; a threshold below that error fails the run.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../common/map_align.h"
#include "../common/voxel_moments.h"

using namespace madicp_host;

struct P { int64_t x, y, z; };
enum Kind { kPoint, kLine, kPlane, kSolid };
struct Shape { const char* name; Kind kind; std::vector<P> d; };  // offsets with smallest coordinate 0 on every axis

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static std::vector<Shape> shapes() {
  std::vector<Shape> out;
  auto line = [](int n, int64_t step, P dir) {
    std::vector<P> v;
    for (int k = 0; k < n; ++k) v.push_back({k * step * dir.x, k * step * dir.y, k * step * dir.z});
    return v;
  };
  out.push_back({"one", kPoint, {{0, 0, 0}}});
  out.push_back({"two", kLine, {{0, 0, 0}, {300, 200, 100}}});
  out.push_back({"identical3", kPoint, std::vector<P>(3, P{0, 0, 0})});
  out.push_back({"identical4096", kPoint, std::vector<P>(4096, P{0, 0, 0})});
  for (int n : {3, 100}) {
    const int64_t step = n == 3 ? 9000 : 190;
    out.push_back({"line_axis", kLine, line(n, step, {1, 0, 0})});
    out.push_back({"line_face", kLine, line(n, step, {1, 1, 0})});
    out.push_back({"line_531", kLine, line(n, step / 5, {5, 3, 1})});
  }
  std::vector<P> axis, tilted, floored;
  for (int64_t i = 0; i < 10; ++i)
    for (int64_t j = 0; j < 10; ++j) {
      axis.push_back({100 * i, 130 * j, 0});
      tilted.push_back({100 * i, 130 * j, 100 * i + 130 * j});
      floored.push_back({37 * i, 53 * j, (37 * i + 53 * j) / 2});
    }
  out.push_back({"plane_axis", kPlane, axis});
  out.push_back({"plane_tilted", kPlane, tilted});
  out.push_back({"plane_floored", kSolid, floored});
  out.push_back({"triangle", kPlane, {{0, 700, 0}, {900, 0, 200}, {300, 400, 1100}}});
  out.push_back({"square", kPlane, {{0, 0, 0}, {20000, 0, 0}, {0, 20000, 0}, {20000, 20000, 0}}});
  out.push_back({"tetra", kSolid, {{0, 700, 0}, {900, 0, 200}, {300, 400, 1100}, {1000, 1000, 50}}});
  std::vector<P> cube, top;
  for (int k = 0; k < 8; ++k) cube.push_back({20000 * (k & 1), 20000 * ((k >> 1) & 1), 20000 * (k >> 2)});
  out.push_back({"cube", kSolid, cube});
  uint32_t seed = 7;
  for (int k = 0; k < 100000; ++k) top.push_back({(lcg(seed) >> 8) % 3, (lcg(seed) >> 8) % 3, (lcg(seed) >> 8) % 3});
  out.push_back({"top_cube_100000", kSolid, top});
  out.push_back({"three_and_one", kLine, {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {65535, 65535, 65535}}});
  return out;
}

static int fail(const char* what, const char* name, int variant, double a, double b) {
  std::fprintf(stderr, "%s (variant %d): %s (%.9g, %.9g)\n", name, variant, what, a, b);
  return 1;
}

int main() {
  const double voxel = 0.5;
  const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  const uint64_t keys[3] = {0, 0x7fffffffffffffffull, (uint64_t(1048575) << 42) | (uint64_t(1048575) << 21) | 1048575};
  int surfels = 0, admitted = 0, negative = 0;
  double worst_share = 0.0, worst_floor = 0.0, worst_of_threshold = 0.0;
  for (const Shape& s : shapes()) {
    int64_t hi[3] = {0, 0, 0};
    for (const P& p : s.d) {
      const int64_t c[3] = {p.x, p.y, p.z};
      for (int a = 0; a < 3; ++a) hi[a] = c[a] > hi[a] ? c[a] : hi[a];
    }
    for (int where = 0; where < 3; ++where)
      for (int variant = 0; variant < 12; ++variant) {
        uint64_t* M = static_cast<uint64_t*>(std::malloc(sizeof(uint64_t) * kMomentWords));
        for (int k = 0; k < kMomentWords; ++k) M[k] = 0;
        for (const P& p : s.d) {
          const int64_t c[3] = {p.x, p.y, p.z};
          uint32_t w[3];
          for (int a = 0; a < 3; ++a) {
            const int from = perms[variant / 2][a];
            const int64_t room = 65535 - hi[from];
            const int64_t v = c[from] + (where == 0 ? 0 : where == 1 ? room / 2 : room);
            if (v < 0 || v > 65535) return fail("an offset outside the voxel", s.name, variant, static_cast<double>(v), 0);
            w[a] = static_cast<uint32_t>(variant % 2 ? 65535 - v : v);
          }
          uint64_t t[9];
          moment_terms(w, t);
          M[0] += 1;
          for (int k = 0; k < 9; ++k) M[1 + k] += t[k];
        }
        float* centroid = static_cast<float*>(std::malloc(3 * sizeof(float)));
        float* normal = static_cast<float*>(std::malloc(3 * sizeof(float)));
        float* eig = static_cast<float*>(std::malloc(3 * sizeof(float)));
        uint32_t count = 0;
        map_surfel(M, keys[(where + variant) % 3], voxel, centroid, normal, eig, &count);
        ++surfels;
        if (s.kind == kPoint || s.kind == kLine) {  // the solve WITHOUT the rule, where eigenvalues 0 and 1 are exactly zero
          double m[3], w[3], V[9];
          for (int a = 0; a < 3; ++a) m[a] = static_cast<double>(M[1 + a]) / static_cast<double>(M[0]);
          const double zero_at = surfel_solve(M, m, w, V);
          const double floor = (zero_at - kSurfelZeroShare * w[2]) / kSurfelZeroFloor;
          for (int i = 0; i < 2; ++i) {
            const double err = std::fabs(w[i]);
            if (err > zero_at) return fail("the rule's threshold is below the solver's error on a zero eigenvalue", s.name, variant, err, zero_at);
            if (err > 0.0 && err > worst_of_threshold * zero_at) worst_of_threshold = err / zero_at;
            // charged to the share where the floor is under a thousandth of the error, else to the floor (after the measured share)
            if (floor < 1e-3 * err) {
              if (err > worst_share * w[2]) worst_share = err / w[2];
            } else if (floor > 0.0 && err - 3.73e-9 * w[2] > worst_floor * floor) {
              worst_floor = (err - 3.73e-9 * w[2]) / floor;
            }
            negative += w[i] < 0.0;
          }
        }
        if (count != s.d.size()) return fail("count", s.name, variant, count, static_cast<double>(s.d.size()));
        double nn = 0;
        for (int a = 0; a < 3; ++a) {
          if (!std::isfinite(centroid[a]) || !std::isfinite(normal[a]) || !std::isfinite(eig[a])) return fail("not finite", s.name, variant, a, 0);
          if (std::signbit(eig[a])) return fail("a negative eigenvalue", s.name, variant, a, eig[a]);
          nn += static_cast<double>(normal[a]) * static_cast<double>(normal[a]);
        }
        if (!(eig[0] <= eig[1] && eig[1] <= eig[2])) return fail("eigenvalues not ascending", s.name, variant, eig[0], eig[1]);
        if (count < 3 ? nn != 0.0 : std::fabs(nn - 1.0) > 1.04e-7) return fail("the normal's length", s.name, variant, nn, count);
        if (s.kind == kPoint && eig[2] != 0.0f) return fail("identical points with a spread", s.name, variant, eig[2], 0);
        if (s.kind == kLine && !(eig[1] == 0.0f && eig[2] > 0.0f)) return fail("a line's spectrum is not 0, 0, +", s.name, variant, eig[1], eig[2]);
        if (s.kind == kPlane && !(eig[0] == 0.0f && eig[1] > 0.0f)) return fail("a plane's spectrum is not 0, +, +", s.name, variant, eig[0], eig[1]);
        for (double flat : {1.0, 0.3, 1e-3})
          for (uint32_t min_count : {3u, count, count + 1u}) {
            if (min_count < 3) continue;
            const bool in = align_inlier(true, count, eig, min_count, flat);
            admitted += in;
            if (align_inlier(false, count, eig, min_count, flat)) return fail("an inlier that is not within", s.name, variant, flat, min_count);
            if (in && (s.kind == kPoint || s.kind == kLine)) return fail("a voxel without a plane is an inlier", s.name, variant, flat, eig[1]);
            if (in && count < min_count) return fail("an inlier below min_count", s.name, variant, count, min_count);
            if (!in && count >= min_count && (s.kind == kPlane || (s.kind == kSolid && flat == 1.0)))
              return fail("a plane is refused", s.name, variant, flat, eig[1]);
          }
        std::free(M);
        std::free(centroid);
        std::free(normal);
        std::free(eig);
      }
  }
  std::printf("%d surfels clean, %d decisions admitted\n", surfels, admitted);
  std::printf("without the zero rule: %d exactly-zero eigenvalues come out negative; their worst error %.3e of w2, %.3f floors, "
              "%.4f of the rule's threshold\n", negative, worst_share, worst_floor, worst_of_threshold);
  return 0;
}
