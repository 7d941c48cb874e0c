// Stand-alone check of the host voxel map's free-space clearing (madicp_host_map_clear_rays: csrc/host/voxel_map.cpp + voxel_map.h)
// under AddressSanitizer and UndefinedBehaviorSanitizer: compiled and run by tests/test_map_clear_sanitized.py.  Every cloud lives in
// a heap buffer of EXACTLY n rows and every download goes into a buffer of EXACTLY the rows the map holds: a read past the cloud or
// a write past the last row ends the program with the sanitizer's report.  The results are held to the obvious reading of the
// rule: a brute-force list of (row, cell, word), and per clearing two plain lists of cells — sampled and occupied — searched linearly.
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

struct Cell {
  int64_t c[3];
  bool operator==(const Cell& o) const { return c[0] == o.c[0] && c[1] == o.c[1] && c[2] == o.c[2]; }
};
struct Row {
  float p[3];
  Cell cell;
  uint32_t word;
};

static bool cell_of(const double* q, double voxel, Cell* out) {
  for (int a = 0; a < 3; ++a) {
    const double f = std::floor(q[a] / voxel);
    if (!(f >= -1048576.0 && f < 1048576.0)) return false;
    out->c[a] = static_cast<int64_t>(f);
  }
  return true;
}
static bool has(const std::vector<Cell>& v, const Cell& c) {
  for (const Cell& x : v)
    if (x == c) return true;
  return false;
}

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
  const int64_t sizes[] = {1, 2, 63, 64, 65, 255, 257, 1025};
  const double voxels[] = {0.25, 0.5, 50.0};
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  int sets = 0;
  long long total_removed = 0, total_kept = 0;
  for (int64_t n : sizes)
    for (double voxel : voxels)
      for (int with_attr = 0; with_attr < 2; ++with_attr) {
        madicp_host_map* map = nullptr;
        const int rc0 = with_attr ? madicp_host_map_create_attr(voxel, 1, 4 * n, &map) : madicp_host_map_create(voxel, 1, 4 * n, &map);
        if (rc0 != MADICP_OK || !map) return fail("create", sets, 0);
        std::vector<Row> want;
        uint32_t seed = 977u + 31u * static_cast<uint32_t>(n) + static_cast<uint32_t>(sets);
        for (int frame = 0; frame < 3; ++frame) {
          const double t[3] = {1.0 * frame, -0.5 * frame, 0.25 * frame};
          double* xyz = static_cast<double*>(std::malloc(sizeof(double) * 3 * static_cast<size_t>(n)));  // exactly n rows
          uint32_t* attr = static_cast<uint32_t*>(std::malloc(sizeof(uint32_t) * static_cast<size_t>(n)));
          for (int64_t i = 0; i < n; ++i) {
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (unit(seed) - 0.5) * 12.0;
            attr[i] = static_cast<uint32_t>(1000000 * frame + i);
          }
          if (n > 2) xyz[3 * (n / 2)] = NAN;  // a point that is no candidate and has no length
          if (n > 3) xyz[3 * (n / 3) + 1] = INFINITY;
          for (int64_t i = 0; i < n; ++i) {
            Row r;
            double q[3];
            for (int a = 0; a < 3; ++a) {
              q[a] = t[a] + (I[3 * a] * xyz[3 * i] + (I[3 * a + 1] * xyz[3 * i + 1] + I[3 * a + 2] * xyz[3 * i + 2]));
              r.p[a] = static_cast<float>(q[a]);
            }
            bool keep = cell_of(q, voxel, &r.cell);
            for (size_t k = 0; k < want.size() && keep; ++k)
              if (want[k].cell == r.cell) keep = false;
            if (!keep) continue;
            r.word = attr[i];
            want.push_back(r);
          }
          int64_t added = -7, rows = -7;
          const int rc = with_attr ? madicp_host_map_insert_attr(map, xyz, attr, n, I, t, &added, &rows)
                                   : madicp_host_map_insert(map, xyz, n, I, t, &added, &rows);
          if (rc != MADICP_OK || rows != static_cast<int64_t>(want.size())) return fail("insert", sets, frame);
          std::free(attr);
          if (!same(map, with_attr != 0, want)) return fail("rows after the fold", sets, frame);
          // the rays: the folded cloud stretched about the origin (frame 0: looks through most of it), shrunk (frame 1), itself (frame 2)
          const double stretch = frame == 0 ? 1.75 : frame == 1 ? 0.5 : 1.0;
          const double margin = frame == 1 ? 0.125 : 0.0;
          const double o[3] = {0.3125, -0.2, 1.0 / 3.0};
          for (int64_t i = 0; i < 3 * n; ++i) xyz[i] = o[i % 3] + (xyz[i] - o[i % 3]) * stretch;
          // refusals first: they leave everything alone
          const int64_t m = rows, wm = m / 3;
          int64_t removed = -7, left = -7, mark = -7;
          const double obad[3] = {o[0], NAN, o[2]};
          const double Rbad[9] = {1, 0, 0, 0, INFINITY, 0, 0, 0, 1};
          if (madicp_host_map_clear_rays(map, xyz, n, I, t, obad, margin, wm, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 0);
          if (madicp_host_map_clear_rays(map, xyz, n, Rbad, t, o, margin, wm, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 1);
          if (madicp_host_map_clear_rays(map, nullptr, n, I, t, o, margin, wm, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 2);
          if (madicp_host_map_clear_rays(map, xyz, n, I, t, o, -1.0, wm, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 3);
          if (madicp_host_map_clear_rays(map, xyz, n, I, t, o, margin, m + 1, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 4);
          if (madicp_host_map_clear_rays(map, xyz, n, I, t, o, margin, -1, &removed, &left, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 5);
          if (madicp_host_map_clear_rays(map, xyz, n, I, t, o, margin, wm, &removed, nullptr, &mark) != MADICP_ERR_INVALID) return fail("refusal", sets, 6);
          if (removed != -7 || left != -7 || mark != -7 || !same(map, with_attr != 0, want)) return fail("refusal wrote", sets, 7);
          // the rule, the slow way
          std::vector<Cell> sampled, occupied;
          double qo[3];
          for (int a = 0; a < 3; ++a) qo[a] = t[a] + (I[3 * a] * o[0] + (I[3 * a + 1] * o[1] + I[3 * a + 2] * o[2]));
          for (int64_t i = 0; i < n; ++i) {
            double q[3], d[3];
            for (int a = 0; a < 3; ++a) {
              q[a] = t[a] + (I[3 * a] * xyz[3 * i] + (I[3 * a + 1] * xyz[3 * i + 1] + I[3 * a + 2] * xyz[3 * i + 2]));
              d[a] = q[a] - qo[a];
            }
            Cell c;
            if (cell_of(q, voxel, &c) && !has(occupied, c)) occupied.push_back(c);
            const double L = std::sqrt(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]));
            if (!std::isfinite(L) || !(L - margin >= voxel)) continue;
            const double kf = std::floor((L - margin) / voxel);
            const int K = kf < 4096.0 ? static_cast<int>(kf) : 4096;
            for (int k = 1; k <= K; ++k) {
              const double f = (static_cast<double>(k) * voxel) / L;
              const double s[3] = {qo[0] + d[0] * f, qo[1] + d[1] * f, qo[2] + d[2] * f};
              if (cell_of(s, voxel, &c) && (sampled.empty() || !(sampled.back() == c))) sampled.push_back(c);
            }
          }
          std::vector<Row> kept;
          int64_t mark_want = 0;
          for (int64_t j = 0; j < m; ++j) {
            const Row& r = want[static_cast<size_t>(j)];
            if (has(sampled, r.cell) && !has(occupied, r.cell)) continue;
            kept.push_back(r);
            if (j < wm) ++mark_want;
          }
          if (madicp_host_map_clear_rays(map, nullptr, 0, I, t, o, margin, wm, &removed, &left, &mark) != MADICP_OK || removed != 0 || left != m ||
              mark != wm)
            return fail("an empty cloud", sets, frame);
          const int rc2 = madicp_host_map_clear_rays(map, xyz, n, I, t, o, margin, wm, &removed, &left, &mark);
          std::free(xyz);
          if (rc2 != MADICP_OK) return fail("clear_rays", sets, frame);
          if (left != static_cast<int64_t>(kept.size()) || removed != m - left || mark != mark_want) return fail("the clearing's answer", sets, frame);
          total_removed += removed;
          total_kept += left;
          want.swap(kept);
          if (!same(map, with_attr != 0, want)) return fail("rows after the clearing", sets, frame);
        }
        madicp_host_map_destroy(map);
        ++sets;
      }
  if (total_removed < 1000 || total_kept < 1000) return fail("the sets do not exercise both outcomes", sets, total_removed);
  std::printf("map_clear_check: %d sets clean\n", sets);
  return 0;
}
