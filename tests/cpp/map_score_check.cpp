// Stand-alone check of the host voxel map's pose scoring (madicp_host_map_score: csrc/host/voxel_map.cpp + voxel_map.h, the rule of
// csrc/common/export_point.h) under AddressSanitizer and UndefinedBehaviorSanitizer: compiled and run by
// tests/test_map_score_sanitized.py.  Every cloud lives in a heap buffer of EXACTLY n rows, the poses in one of EXACTLY 12 K doubles
// and out_counts in one of EXACTLY 3 K entries: a read or write past any of them ends the program with the sanitizer's report.  The
// counts are held to K separate scoring calls of madicp_host_map_query over the subsampled cloud, copied out on the host.  Maps of
// all four kinds, both reaches, strides around n, and every refusal with a buffer that must stay as it was.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../common/export_point.h"
#include "madicp_host.h"

using namespace madicp_host;

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t& s) { return (lcg(s) >> 8) / 16777216.0; }

static int fail(const char* what, int set, long long i) {
  std::fprintf(stderr, "set %d step %lld: %s\n", set, i, what);
  return 1;
}

template <class T>
static T* exactly(int64_t n) {  // (a zero-byte block is legal, and every access to it is out of bounds)
  return static_cast<T*>(std::malloc(sizeof(T) * static_cast<size_t>(n)));
}

constexpr uint64_t kSentinel = 0x7777777777777777ull;

static int refusals(madicp_host_map* map, int set) {
  const double inf = std::numeric_limits<double>::infinity();
  const int64_t n = 9, K = 3;
  double* cloud = exactly<double>(3 * n);
  double* poses = exactly<double>(12 * K);
  uint64_t* counts = exactly<uint64_t>(3 * K);
  for (int64_t i = 0; i < 3 * n; ++i) cloud[i] = 0.1 * static_cast<double>(i);
  auto reset = [&]() {
    for (int64_t k = 0; k < K; ++k) {
      const double X[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5 * static_cast<double>(k), 0, 0};
      std::memcpy(poses + 12 * k, X, sizeof(X));
    }
    for (int64_t i = 0; i < 3 * K; ++i) counts[i] = kSentinel;
  };
  auto untouched = [&]() {
    for (int64_t i = 0; i < 3 * K; ++i)
      if (counts[i] != kSentinel) return false;
    return true;
  };
  int step = 0;
  auto refused = [&](int rc) {
    ++step;
    return rc == MADICP_ERR_INVALID && untouched();
  };
  reset();
  if (!refused(madicp_host_map_score(nullptr, cloud, n, poses, K, 1, 1.0, 1, counts))) return fail("null map", set, step);
  if (!refused(madicp_host_map_score(map, nullptr, n, poses, K, 1, 1.0, 1, counts))) return fail("null cloud", set, step);
  if (!refused(madicp_host_map_score(map, cloud, n, nullptr, K, 1, 1.0, 1, counts))) return fail("null poses", set, step);
  if (madicp_host_map_score(map, cloud, n, poses, K, 1, 1.0, 1, nullptr) != MADICP_ERR_INVALID) return fail("null counts", set, step);
  if (!refused(madicp_host_map_score(map, cloud, -1, poses, K, 1, 1.0, 1, counts))) return fail("n < 0", set, step);
  if (!refused(madicp_host_map_score(map, cloud, n, poses, 0, 1, 1.0, 1, counts))) return fail("K = 0", set, step);
  if (!refused(madicp_host_map_score(map, cloud, n, poses, -2, 1, 1.0, 1, counts))) return fail("K < 0", set, step);
  if (!refused(madicp_host_map_score(map, cloud, n, poses, kScoreMaxPoses + 1, 1, 1.0, 1, counts))) return fail("K too large", set, step);
  for (int reach : {-1, 2, 27})
    if (!refused(madicp_host_map_score(map, cloud, n, poses, K, reach, 1.0, 1, counts))) return fail("reach", set, step);
  for (double md : {std::nan(""), -1.0, -inf})
    if (!refused(madicp_host_map_score(map, cloud, n, poses, K, 1, md, 1, counts))) return fail("max_dist", set, step);
  for (int64_t stride : {int64_t(0), int64_t(-1), std::numeric_limits<int64_t>::min()})
    if (!refused(madicp_host_map_score(map, cloud, n, poses, K, 1, 1.0, stride, counts))) return fail("stride", set, step);
  for (double bad : {std::nan(""), inf, -inf})
    for (int64_t at : {int64_t(0), 12 * (K - 1) + 11, 12 * (K - 1) + 4}) {
      reset();
      poses[at] = bad;
      if (!refused(madicp_host_map_score(map, cloud, n, poses, K, 1, 1.0, 1, counts))) return fail("a non-finite pose entry", set, at);
    }
  reset();
  if (madicp_host_map_score(map, nullptr, 0, poses, K, 1, 1.0, 1, counts) != MADICP_OK) return fail("n = 0 is legal", set, step);
  for (int64_t i = 0; i < 3 * K; ++i)
    if (counts[i] != 0) return fail("n = 0 gives zeros", set, i);
  if (madicp_host_map_score(map, cloud, n, poses, K, 0, inf, std::numeric_limits<int64_t>::max(), counts) != MADICP_OK)
    return fail("the largest stride is legal", set, step);
  if (counts[0] != 1) return fail("the largest stride scores the first point alone", set, static_cast<long long>(counts[0]));
  std::free(cloud);
  std::free(poses);
  std::free(counts);
  return 0;
}

int main() {
  const double voxel = 0.5;
  const double inf = std::numeric_limits<double>::infinity();
  int sets = 0;
  for (int set = 0; set < 32; ++set) {
    uint32_t seed = 4000u + set;
    const int kind = set % 4;  // plain, attr, evidence (+ attr), moments
    madicp_host_map* map = nullptr;
    int rc = kind == 0   ? madicp_host_map_create(voxel, 1 + set, 1 << 20, &map)
             : kind == 1 ? madicp_host_map_create_attr(voxel, 1 + set, 1 << 20, &map)
             : kind == 2 ? madicp_host_map_create_ev(voxel, 1 + set, 1 << 20, 1, 2, 1, 6, &map)
                         : madicp_host_map_create_mom(voxel, 1 + set, 1 << 20, 0, nullptr, 4, &map);
    if (rc != MADICP_OK) return fail("create", set, rc);
    const double kI[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kZ[3] = {0, 0, 0};
    {  // the map: a blob around the origin
      const int64_t m = 150 + 13 * set;
      double* pts = exactly<double>(3 * m);
      for (int64_t i = 0; i < 3 * m; ++i) pts[i] = (unit(seed) - 0.5) * 6.0;
      int64_t added = 0, rows = 0;
      rc = madicp_host_map_insert(map, pts, m, kI, kZ, &added, &rows);
      std::free(pts);
      if (rc != MADICP_OK || rows < 20) return fail("fold", set, rc);
    }
    const int64_t sizes[] = {0, 1, 2, 63, 64, 65, 200};
    const int64_t n = sizes[set % 7], K = 1 + (set * 5) % 9;
    double* cloud = exactly<double>(3 * n);
    for (int64_t i = 0; i < 3 * n; ++i) cloud[i] = (unit(seed) - 0.5) * 7.0;
    if (n > 4) {  // points that are no candidate, and points exactly on voxel faces
      cloud[3] = std::nan("");
      cloud[7] = inf;
      cloud[9] = 1.0, cloud[10] = -0.5, cloud[11] = 0.0;
    }
    double* poses = exactly<double>(12 * K);
    for (int64_t k = 0; k < K; ++k) {
      const double a = k == 0 ? 0.0 : (unit(seed) - 0.5) * 0.6, c = std::cos(a), s = std::sin(a);
      const double far = k == 2 ? 3e6 : 0.0;  // (pose 2 throws every point outside the key range)
      const double X[12] = {c, -s, 0, s, c, 0, 0, 0, 1, far + (k ? unit(seed) - 0.5 : 0.0), k ? 0.5 * static_cast<double>(k % 3) : 0.0, 0};
      std::memcpy(poses + 12 * k, X, sizeof(X));
    }
    if (K >= 4) std::memcpy(poses + 12 * (K - 1), poses, 12 * sizeof(double));  // the same pose twice
    const int64_t strides[] = {1, 2, 7, n > 0 ? n : 1, n + 1};
    for (int64_t stride : strides)
      for (int reach = 0; reach < 2; ++reach)
        for (double md : {0.0, 0.3, inf}) {
          uint64_t* counts = exactly<uint64_t>(3 * K);
          if (madicp_host_map_score(map, n ? cloud : nullptr, n, poses, K, reach, md, stride, counts) != MADICP_OK)
            return fail("score", set, stride);
          const int64_t n_sub = n == 0 ? 0 : (n - 1) / stride + 1;
          double* sub = exactly<double>(3 * n_sub);
          for (int64_t s = 0; s < n_sub; ++s) std::memcpy(sub + 3 * s, cloud + 3 * s * stride, 3 * sizeof(double));
          for (int64_t k = 0; k < K; ++k) {
            uint64_t one[3] = {9, 9, 9};
            if (madicp_host_map_query(map, n_sub ? sub : nullptr, n_sub, poses + 12 * k, poses + 12 * k + 9, reach, md, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, 0, one) != MADICP_OK)
              return fail("the scoring query", set, k);
            if (std::memcmp(one, counts + 3 * k, sizeof(one)) != 0) return fail("counts differ from the scoring query's", set, k);
            if (k == 2 && counts[3 * k] != 0) return fail("a pose outside the key range has candidates", set, k);
          }
          if (K >= 4 && std::memcmp(counts, counts + 3 * (K - 1), 3 * sizeof(uint64_t)) != 0) return fail("the same pose twice", set, K);
          std::free(sub);
          std::free(counts);
        }
    std::free(cloud);
    std::free(poses);
    if (refusals(map, set)) return 1;
    madicp_host_map_destroy(map);
    ++sets;
  }
  std::printf("%d sets clean\n", sets);
  return 0;
}
