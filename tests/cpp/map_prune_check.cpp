// Stand-alone check of the host voxel map's prune (madicp_host_map_prune: csrc/host/voxel_map.cpp + voxel_map.h) under
// AddressSanitizer and UndefinedBehaviorSanitizer: compiled and run by tests/test_map_prune_sanitized.py.  Every cloud lives in a
// heap buffer of EXACTLY n rows and every download goes into a buffer of EXACTLY the rows the map holds: a read past the cloud or
// a write past the last row ends the program with the sanitizer's report.  The results are held to the obvious reading of the
// rule: a brute-force list of (row, cell, word) over the same positions, filtered in place by the distance of the float row.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "madicp_host.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t& s) { return (double)(lcg(s) >> 8) / 16777216.0; }  // [0, 1)

static int fail(const char* what, int set, long long i) {
  std::fprintf(stderr, "set %d step %lld: %s\n", set, i, what);
  return 1;
}

struct Row {
  float p[3];
  int64_t c[3];
  uint32_t word;
};

// the map's rows and words into buffers of exactly its size, compared with `want`
static bool same(madicp_host_map* map, bool with_attr, const std::vector<Row>& want) {
  int64_t m = -7;
  if (madicp_host_map_size(map, &m) != MADICP_OK || m != static_cast<int64_t>(want.size())) return false;
  float* rows = static_cast<float*>(std::malloc(sizeof(float) * 3 * static_cast<size_t>(m > 0 ? m : 1)));
  uint32_t* words = static_cast<uint32_t*>(std::malloc(sizeof(uint32_t) * static_cast<size_t>(m > 0 ? m : 1)));
  int64_t got = -7;
  bool ok = madicp_host_map_download_f32(map, 0, rows, m, &got) == MADICP_OK && got == m;
  if (ok && with_attr) ok = madicp_host_map_download_attr(map, 0, words, m, &got) == MADICP_OK && got == m;
  for (int64_t j = 0; ok && j < m; ++j) {
    ok = std::memcmp(rows + 3 * j, want[static_cast<size_t>(j)].p, sizeof(float) * 3) == 0;
    if (ok && with_attr) ok = words[j] == want[static_cast<size_t>(j)].word;
  }
  std::free(rows);
  std::free(words);
  return ok;
}

int main() {
  const int64_t sizes[] = {1, 2, 63, 64, 65, 255, 257, 1024, 1025, 3000};
  const double voxels[] = {1e-3, 0.5, 50.0};
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  int sets = 0;
  for (int64_t n : sizes)
    for (double voxel : voxels)
      for (int with_attr = 0; with_attr < 2; ++with_attr) {
        madicp_host_map* map = nullptr;
        const int rc0 = with_attr ? madicp_host_map_create_attr(voxel, 1, 4 * n, &map) : madicp_host_map_create(voxel, 1, 4 * n, &map);
        if (rc0 != MADICP_OK || !map) return fail("create", sets, 0);
        std::vector<Row> want;
        uint32_t seed = 4177u + 29u * static_cast<uint32_t>(n) + static_cast<uint32_t>(sets);
        for (int frame = 0; frame < 4; ++frame) {
          const double t[3] = {3.0 * frame, -1.5 * frame, 0.25 * frame};
          double* xyz = static_cast<double*>(std::malloc(sizeof(double) * 3 * static_cast<size_t>(n)));  // exactly n rows
          uint32_t* attr = static_cast<uint32_t*>(std::malloc(sizeof(uint32_t) * static_cast<size_t>(n)));
          for (int64_t i = 0; i < n; ++i) {
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (unit(seed) - 0.5) * 30.0;
            attr[i] = static_cast<uint32_t>(1000000 * frame + i);
          }
          if (n > 2) xyz[3 * (n / 2)] = NAN;  // a row that is no candidate
          for (int64_t i = 0; i < n; ++i) {
            Row r;
            bool keep = true;
            for (int a = 0; a < 3; ++a) {
              const double q = t[a] + (I[3 * a] * xyz[3 * i] + (I[3 * a + 1] * xyz[3 * i + 1] + I[3 * a + 2] * xyz[3 * i + 2]));
              const double f = std::floor(q / voxel);
              if (!(f >= -1048576.0 && f < 1048576.0)) { keep = false; break; }
              r.c[a] = static_cast<int64_t>(f);
              r.p[a] = static_cast<float>(q);
            }
            for (size_t k = 0; k < want.size() && keep; ++k)
              if (want[k].c[0] == r.c[0] && want[k].c[1] == r.c[1] && want[k].c[2] == r.c[2]) keep = false;
            if (!keep) continue;
            r.word = attr[i];
            want.push_back(r);
          }
          int64_t added = -7, rows = -7;
          const int rc = with_attr ? madicp_host_map_insert_attr(map, xyz, attr, n, I, t, &added, &rows)
                                   : madicp_host_map_insert(map, xyz, n, I, t, &added, &rows);
          if (rc != MADICP_OK || rows != static_cast<int64_t>(want.size())) return fail("insert", sets, frame);
          std::free(xyz);
          std::free(attr);
          if (!same(map, with_attr != 0, want)) return fail("rows after the fold", sets, frame);
          // refusals first: they leave everything alone
          const int64_t m = rows, wm = m / 3;
          int64_t removed = -7, left = -7, mark = -7;
          const double c[3] = {t[0] + 0.3125, t[1], t[2] - 1.0 / 3.0};
          const double cbad[3] = {c[0], NAN, c[2]};
          if (madicp_host_map_prune(map, cbad, 5.0, wm, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 0);
          if (madicp_host_map_prune(map, nullptr, 5.0, wm, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 1);
          if (madicp_host_map_prune(map, c, 0.0, wm, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 2);
          if (madicp_host_map_prune(map, c, 1e200, wm, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 3);
          if (madicp_host_map_prune(map, c, 5.0, m + 1, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 4);
          if (madicp_host_map_prune(map, c, 5.0, -1, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 5);
          if (madicp_host_map_prune(map, c, 5.0, wm, nullptr, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 6);
          if (removed != -7 || left != -7 || mark != -7 || !same(map, with_attr != 0, want)) return fail("refusal wrote", sets, 7);
          // the prune: radius 12 on even frames, 1e-3 (next to nothing stays) on frame 1, everything on frame 3
          const double radius = frame == 1 ? 1e-3 : frame == 3 ? 1e6 : 12.0;
          const double r2 = radius * radius;
          std::vector<Row> kept;
          int64_t mark_want = 0;
          for (int64_t j = 0; j < m; ++j) {
            const Row& r = want[static_cast<size_t>(j)];
            const double dx = (double)r.p[0] - c[0], dy = (double)r.p[1] - c[1], dz = (double)r.p[2] - c[2];
            if (!(dx * dx + (dy * dy + dz * dz) <= r2)) continue;
            kept.push_back(r);
            if (j < wm) ++mark_want;
          }
          if (madicp_host_map_prune(map, c, radius, wm, &removed, &left, &mark) != MADICP_OK) return fail("prune", sets, frame);
          if (left != static_cast<int64_t>(kept.size()) || removed != m - left || mark != mark_want) return fail("prune's answer", sets, frame);
          want.swap(kept);
          if (!same(map, with_attr != 0, want)) return fail("rows after the prune", sets, frame);
        }
        // to empty, then a prune of the empty map
        int64_t removed = -7, left = -7, mark = -7;
        const double far[3] = {1e5, 0, 0};
        const int64_t m = static_cast<int64_t>(want.size());
        if (madicp_host_map_prune(map, far, 1.0, m, &removed, &left, &mark) != MADICP_OK || removed != m || left != 0 || mark != 0)
          return fail("prune to empty", sets, 0);
        if (madicp_host_map_prune(map, far, 1.0, 0, &removed, &left, &mark) != MADICP_OK || removed != 0 || left != 0 || mark != 0)
          return fail("prune of an empty map", sets, 0);
        want.clear();
        if (!same(map, with_attr != 0, want)) return fail("rows of the empty map", sets, 0);
        madicp_host_map_destroy(map);
        ++sets;
      }
  std::printf("map_prune_check: %d sets clean\n", sets);
  return 0;
}
