// Stand-alone check of the host voxel map's removal log (madicp_host_map_track_removed / _removed_count / _take_removed and
// _download_keys / _download_rows: csrc/host/voxel_map.cpp + voxel_map.h) under AddressSanitizer and UndefinedBehaviorSanitizer:
// compiled and run by tests/test_map_removed_sanitized.py.  Every cloud lives in a heap buffer of EXACTLY n rows, every take goes
// into buffers of EXACTLY the entries the log holds and every download into buffers of EXACTLY the rows the map holds: a write past
// the last entry ends the program with the sanitizer's report.  The results are held to the obvious reading of the rule: a
// brute-force list of (key, row, word) over the same positions, from which what leaves below the watermark is moved to a list.
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
  uint64_t key;
  uint32_t word;
};

template <class T>
static T* exactly(int64_t n) {  // (a zero-byte block is legal, and every write to it is out of bounds)
  return static_cast<T*>(std::malloc(sizeof(T) * static_cast<size_t>(n)));
}

static bool same_rows(const std::vector<Row>& want, const uint64_t* keys, const float* rows, const uint32_t* words) {
  for (size_t j = 0; j < want.size(); ++j) {
    if (keys && keys[j] != want[j].key) return false;
    if (std::memcmp(rows + 3 * j, want[j].p, sizeof(float) * 3) != 0) return false;
    if (words && words[j] != want[j].word) return false;
  }
  return true;
}

// the map's columns through _download_rows and through _download_keys into buffers of exactly its size, compared with `want`
static bool same_map(madicp_host_map* map, bool with_attr, const std::vector<Row>& want) {
  int64_t m = -7, got = -7;
  if (madicp_host_map_size(map, &m) != MADICP_OK || m != static_cast<int64_t>(want.size())) return false;
  float* rows = exactly<float>(3 * m);
  uint64_t *keys = exactly<uint64_t>(m), *keys2 = exactly<uint64_t>(m);
  uint32_t* words = with_attr ? exactly<uint32_t>(m) : nullptr;
  bool ok = madicp_host_map_download_rows(map, 0, rows, keys, words, m, &got) == MADICP_OK && got == m;
  ok = ok && madicp_host_map_download_keys(map, 0, keys2, m, &got) == MADICP_OK && got == m;
  ok = ok && (m == 0 || std::memcmp(keys, keys2, sizeof(uint64_t) * static_cast<size_t>(m)) == 0) && same_rows(want, keys, rows, words);
  if (ok && m > 1) {  // a window that starts inside the map
    ok = madicp_host_map_download_rows(map, m - 1, rows, nullptr, nullptr, 1, &got) == MADICP_OK && got == 1 &&
         std::memcmp(rows, want.back().p, sizeof(float) * 3) == 0;
  }
  std::free(rows);
  std::free(keys);
  std::free(keys2);
  std::free(words);
  return ok;
}

// the log taken into buffers of exactly its length, compared with `want` (which is emptied); one short first: nothing taken
static bool take(madicp_host_map* map, bool with_attr, std::vector<Row>& want) {
  int64_t n = -7, got = -7;
  if (madicp_host_map_removed_count(map, &n) != MADICP_OK || n != static_cast<int64_t>(want.size())) return false;
  uint64_t* keys = exactly<uint64_t>(n);
  float* rows = exactly<float>(3 * n);
  uint32_t* words = with_attr ? exactly<uint32_t>(n) : nullptr;
  bool ok = true;
  if (n > 0) {
    ok = madicp_host_map_take_removed(map, keys, rows, words, n - 1, &got) == MADICP_ERR_CAPACITY && got == n;
    int64_t still = -7;
    ok = ok && madicp_host_map_removed_count(map, &still) == MADICP_OK && still == n;
  }
  ok = ok && madicp_host_map_take_removed(map, keys, rows, words, n, &got) == MADICP_OK && got == n && same_rows(want, keys, rows, words);
  int64_t after = -7;
  ok = ok && madicp_host_map_removed_count(map, &after) == MADICP_OK && after == 0;
  std::free(keys);
  std::free(rows);
  std::free(words);
  want.clear();
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
        if (madicp_host_map_track_removed(map, 1) != MADICP_OK) return fail("track", sets, 0);
        std::vector<Row> want, log;
        uint32_t seed = 977u + 31u * static_cast<uint32_t>(n) + static_cast<uint32_t>(sets);
        for (int frame = 0; frame < 4; ++frame) {
          const double t[3] = {3.0 * frame, -1.5 * frame, 0.25 * frame};
          double* xyz = exactly<double>(3 * n);  // exactly n rows
          uint32_t* attr = exactly<uint32_t>(n);
          for (int64_t i = 0; i < n; ++i) {
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (unit(seed) - 0.5) * 30.0;
            attr[i] = static_cast<uint32_t>(1000000 * frame + i);
          }
          if (n > 2) xyz[3 * (n / 2)] = NAN;  // a row that is no candidate
          for (int64_t i = 0; i < n; ++i) {
            Row r;
            r.key = 0;
            bool keep = true;
            for (int a = 0; a < 3; ++a) {
              const double q = t[a] + (I[3 * a] * xyz[3 * i] + (I[3 * a + 1] * xyz[3 * i + 1] + I[3 * a + 2] * xyz[3 * i + 2]));
              const double f = std::floor(q / voxel);
              if (!(f >= -1048576.0 && f < 1048576.0)) { keep = false; break; }
              r.key |= static_cast<uint64_t>(static_cast<int64_t>(f) + 1048576) << (21 * a);
              r.p[a] = static_cast<float>(q);
            }
            for (size_t k = 0; k < want.size() && keep; ++k)
              if (want[k].key == r.key) keep = false;
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
          if (!same_map(map, with_attr != 0, want)) return fail("rows after the fold", sets, frame);
          // the prune: radius 12 on even frames, 1e-3 (next to nothing stays) on frame 1, everything stays on frame 3; the watermark
          // is a third of the rows, all of them on frame 1
          const int64_t m = rows, wm = frame == 1 ? m : m / 3;
          const double c[3] = {t[0] + 0.3125, t[1], t[2] - 1.0 / 3.0};
          const double radius = frame == 1 ? 1e-3 : frame == 3 ? 1e6 : 12.0;
          const double r2 = radius * radius;
          std::vector<Row> kept;
          int64_t mark_want = 0;
          for (int64_t j = 0; j < m; ++j) {
            const Row& r = want[static_cast<size_t>(j)];
            const double dx = (double)r.p[0] - c[0], dy = (double)r.p[1] - c[1], dz = (double)r.p[2] - c[2];
            if (!(dx * dx + (dy * dy + dz * dz) <= r2)) {
              if (j < wm) log.push_back(r);
              continue;
            }
            kept.push_back(r);
            if (j < wm) ++mark_want;
          }
          int64_t removed = -7, left = -7, mark = -7;
          if (madicp_host_map_prune(map, c, radius, wm, &removed, &left, &mark) != MADICP_OK) return fail("prune", sets, frame);
          if (left != static_cast<int64_t>(kept.size()) || removed != m - left || mark != mark_want) return fail("prune's answer", sets, frame);
          want.swap(kept);
          if (!same_map(map, with_attr != 0, want)) return fail("rows after the prune", sets, frame);
          int64_t count = -7;
          if (madicp_host_map_removed_count(map, &count) != MADICP_OK || count != static_cast<int64_t>(log.size())) return fail("count", sets, frame);
          // taken after frames 1 and 3 only: the removals of two prunes in one log
          if (frame % 2 == 1 && !take(map, with_attr != 0, log)) return fail("take", sets, frame);
        }
        // a clearing along +x from far outside through everything, watermark = rows: what it removes is logged behind nothing
        {
          const int64_t m = static_cast<int64_t>(want.size());
          int64_t removed = -7, left = -7, mark = -7, count = -7;
          double* ray = exactly<double>(3);
          ray[0] = 400.0, ray[1] = want.empty() ? 0.0 : (double)want[0].p[1], ray[2] = want.empty() ? 0.0 : (double)want[0].p[2];
          const double origin[3] = {-400.0, ray[1], ray[2]}, zero[3] = {0, 0, 0};
          if (madicp_host_map_clear_rays(map, ray, 1, I, zero, origin, 0.0, m, &removed, &left, &mark) != MADICP_OK)
            return fail("clearing", sets, 0);
          std::free(ray);
          if (removed + left != m || mark != left) return fail("clearing's answer", sets, 0);
          if (madicp_host_map_removed_count(map, &count) != MADICP_OK || count != removed) return fail("count after the clearing", sets, 0);
          uint64_t* keys = exactly<uint64_t>(count);
          float* rows = exactly<float>(3 * count);
          int64_t got = -7;
          if (madicp_host_map_take_removed(map, keys, rows, nullptr, count, &got) != MADICP_OK || got != count) return fail("take", sets, 1);
          for (int64_t e = 0; e < count; ++e) {  // every entry is a row the map held, and holds no more
            size_t j = 0;
            while (j < want.size() && want[j].key != keys[e]) ++j;
            if (j == want.size() || std::memcmp(want[j].p, rows + 3 * e, sizeof(float) * 3) != 0) return fail("the clearing's log", sets, e);
            want.erase(want.begin() + static_cast<long>(j));
          }
          std::free(keys);
          std::free(rows);
          if (!same_map(map, with_attr != 0, want)) return fail("rows after the clearing", sets, 0);
        }
        // tracking off frees the log; a take is then refused; _clear empties a log
        int64_t removed = -7, left = -7, mark = -7, count = -7, got = -7;
        const double far[3] = {1e5, 0, 0};
        const int64_t m = static_cast<int64_t>(want.size());
        if (madicp_host_map_prune(map, far, 1.0, m, &removed, &left, &mark) != MADICP_OK || removed != m || left != 0) return fail("to empty", sets, 0);
        if (madicp_host_map_removed_count(map, &count) != MADICP_OK || count != m) return fail("count of the last prune", sets, 0);
        if (madicp_host_map_clear(map) != MADICP_OK || madicp_host_map_removed_count(map, &count) != MADICP_OK || count != 0)
          return fail("clear empties the log", sets, 0);
        if (madicp_host_map_track_removed(map, 0) != MADICP_OK) return fail("track off", sets, 0);
        uint64_t* none_k = exactly<uint64_t>(0);
        float* none_x = exactly<float>(0);
        if (madicp_host_map_take_removed(map, none_k, none_x, nullptr, 0, &got) != MADICP_ERR_INVALID || got != -7) return fail("take, off", sets, 0);
        std::free(none_k);
        std::free(none_x);
        madicp_host_map_destroy(map);
        ++sets;
      }
  std::printf("map_removed_check: %d sets clean\n", sets);
  return 0;
}
