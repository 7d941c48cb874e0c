// Stand-alone check of the host voxel map's query (madicp_host_map_query: csrc/host/voxel_map.cpp + voxel_map.h, the rule of
// csrc/common/export_point.h) under AddressSanitizer and UndefinedBehaviorSanitizer: compiled and run by
// tests/test_map_query_sanitized.py.  Every cloud lives in a heap buffer of EXACTLY n rows and every per-point output goes into a
// buffer of EXACTLY n entries: a write past the last point ends the program with the sanitizer's report.  The answers are held to
// the rule read literally — every point against every row of the downloaded map, the stored key taken apart into its cells — and
// export_key is held to export_key_of_cells(export_cells) over the positions where the two could part: cell faces, both ends of the
// key range, signed zeros, tiny negatives, NaN and the infinities.  Maps of all four kinds, both reaches, every subset of buffers.
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
static T* exactly(int64_t n) {  // (a zero-byte block is legal, and every write to it is out of bounds)
  return static_cast<T*>(std::malloc(sizeof(T) * static_cast<size_t>(n)));
}

static int keys_agree() {
  const double inf = std::numeric_limits<double>::infinity();
  for (double voxel : {0.5, 0.2, 1.0, 3.0}) {
    const double e = 1048576.0 * voxel;
    const double v[] = {0.0, -0.0, voxel, -voxel, 7 * voxel, -7 * voxel, 1e-20, -1e-20, 0.3, -0.3, e, -e, std::nextafter(e, 0.0),
                        std::nextafter(-e, -inf), std::nextafter(-e, 0.0), e - voxel, std::nextafter(e - voxel, 0.0), -e + voxel,
                        std::nan(""), inf, -inf, 1e300, -1e300, 123456.789, -98765.4321};
    const int nv = static_cast<int>(sizeof(v) / sizeof(v[0]));
    long long candidates = 0;
    for (int a = 0; a < nv; ++a)
      for (int b = 0; b < nv; ++b)
        for (int c = 0; c < nv; ++c) {
          const double q[3] = {v[a], v[b], v[c]};
          int32_t cell[3] = {0, 0, 0};
          const bool is = export_cells(q, voxel, cell);
          const uint64_t key = export_key(q, voxel);
          if (is != (key != kExportNoKey)) return fail("export_cells and export_key disagree on a candidate", a, b * nv + c);
          if (!is) continue;
          ++candidates;
          uint64_t own = 0;
          if (export_key_of_cells(cell) != key) return fail("export_key_of_cells(export_cells) is not export_key", a, b * nv + c);
          if (!query_cell_key(cell, kQueryOwnCell, &own) || own != key) return fail("the own cell of the neighbourhood", a, b * nv + c);
          for (int k = 0; k < kQueryCells; ++k) {  // a neighbour has a key iff it is inside the range, and then that cell's
            const int32_t nb[3] = {cell[0] + k % 3 - 1, cell[1] + k / 3 % 3 - 1, cell[2] + k / 9 - 1};
            bool inside = true;
            for (int x = 0; x < 3; ++x) inside = inside && nb[x] >= -1048576 && nb[x] < 1048576;
            uint64_t got = 0;
            if (query_cell_key(cell, k, &got) != inside) return fail("a neighbour outside the key range", a, k);
            if (inside && got != export_key_of_cells(nb)) return fail("a neighbour's key", a, k);
          }
        }
    if (candidates < 1000) return fail("too few candidates", 0, candidates);
  }
  return 0;
}

static const double kI[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kZ[3] = {0, 0, 0};

int main() {
  if (keys_agree()) return 1;
  const double voxel = 0.5;
  const double e = 1048576.0 * voxel;
  int sets = 0;
  for (int set = 0; set < 48; ++set) {
    uint32_t seed = 1000u + set;
    const int kind = set % 4;  // plain, attr, evidence (+ attr), moments
    const bool with_attr = kind == 1 || kind == 2, with_ev = kind == 2;
    madicp_host_map* map = nullptr;
    const uint32_t evp[3] = {2, 1, 6};
    int rc = kind == 0   ? madicp_host_map_create(voxel, 1 + set, 1 << 20, &map)
             : kind == 1 ? madicp_host_map_create_attr(voxel, 1 + set, 1 << 20, &map)
             : kind == 2 ? madicp_host_map_create_ev(voxel, 1 + set, 1 << 20, 1, evp[0], evp[1], evp[2], &map)
                         : madicp_host_map_create_mom(voxel, 1 + set, 1 << 20, 0, nullptr, 4, &map);
    if (rc != MADICP_OK) return fail("create", set, rc);
    const double R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, t[3] = {0.125, -2.5, 0.75};  // (exact: a quarter turn and dyadic offsets)
    const bool posed = set % 3 == 1;
    // folds: a blob around the origin (two per set, the second hits the first's voxels) and, every sixth set, the range's corners
    for (int fold = 0; fold < 2; ++fold) {
      const int64_t m = 40 + 17 * (set % 7) + 100 * fold;
      double* pts = exactly<double>(3 * m);
      uint32_t* words = exactly<uint32_t>(m);
      for (int64_t i = 0; i < m; ++i) {
        for (int a = 0; a < 3; ++a) pts[3 * i + a] = (unit(seed) - 0.5) * 5.0;
        words[i] = 1000u * (fold + 1) + static_cast<uint32_t>(i);
      }
      if (set % 6 == 5 && fold == 0) {
        const double c[4][3] = {{std::nextafter(e, 0.0), std::nextafter(e, 0.0), std::nextafter(e, 0.0)}, {-e, -e, -e}, {-e, 0.25, std::nextafter(e, 0.0)}, {0.0, -0.0, -1e-20}};
        std::memcpy(pts, c, sizeof(c));
      }
      int64_t added = 0, rows = 0;
      rc = madicp_host_map_insert_attr(map, pts, with_attr ? words : nullptr, m, kI, kZ, &added, &rows);
      std::free(pts);
      std::free(words);
      if (rc != MADICP_OK) return fail("insert", set, rc);
    }
    if (set % 4 == 3) {  // rows move: a prune
      const double center[3] = {0.2, -0.1, 0.3};
      int64_t removed = 0, rows = 0, mark = 0;
      if (madicp_host_map_prune(map, center, set % 6 == 5 ? 2.0e6 : 2.2, 0, &removed, &rows, &mark) != MADICP_OK) return fail("prune", set, 0);
    }
    int64_t M = 0, got = 0;
    madicp_host_map_size(map, &M);
    float* rows = exactly<float>(3 * M);
    uint64_t* keys = exactly<uint64_t>(M);
    uint32_t* attr = exactly<uint32_t>(M);
    uint32_t* ev = exactly<uint32_t>(M);
    if (madicp_host_map_download_f32(map, 0, rows, M, &got) != MADICP_OK || got != M) return fail("download", set, 0);
    if (madicp_host_map_download_keys(map, 0, keys, M, &got) != MADICP_OK) return fail("download keys", set, 0);
    if (with_attr && madicp_host_map_download_attr(map, 0, attr, M, &got) != MADICP_OK) return fail("download attr", set, 0);
    if (with_ev && madicp_host_map_download_evidence(map, 0, ev, M, &got) != MADICP_OK) return fail("download evidence", set, 0);

    const int64_t sizes[] = {0, 1, 31, 64, 257};
    for (int64_t n : sizes) {
      double* cloud = exactly<double>(3 * n);
      for (int64_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) cloud[3 * i + a] = (unit(seed) - 0.5) * 6.0;
      if (n >= 31) {  // the edges among them
        const double inf = std::numeric_limits<double>::infinity();
        const double c[8][3] = {{std::nan(""), 0, 0}, {0, inf, 0}, {0, 0, -inf}, {e, 0, 0}, {-e, -e, -e},
                                {std::nextafter(e, 0.0), std::nextafter(e, 0.0), std::nextafter(e, 0.0)}, {-1e-20, -0.0, 0.5}, {-e, 0.5, std::nextafter(e, 0.0) - 0.5}};
        std::memcpy(cloud, c, sizeof(c));
      }
      const double* QR = posed && n < 31 ? R : kI;  // (the edge positions are meant as they stand)
      const double* Qt = posed && n < 31 ? t : kZ;
      for (int reach = 0; reach <= 1; ++reach) {
        const double max_dist = 0.25 + 0.125 * (set % 3), md2 = max_dist * max_dist;
        // the rule read literally
        std::vector<int32_t> want_row(n, -1);
        std::vector<double> want_d2(n, std::numeric_limits<double>::infinity());
        uint64_t want_counts[3] = {0, 0, 0};
        for (int64_t i = 0; i < n; ++i) {
          double q[3];
          int32_t cell[3];
          export_position(cloud + 3 * i, QR, Qt, q);
          if (!export_cells(q, voxel, cell)) continue;
          ++want_counts[0];
          for (int64_t j = 0; j < M; ++j) {
            bool near = true;
            for (int a = 0; a < 3; ++a) {
              const int64_t rc_a = static_cast<int64_t>((keys[j] >> (21 * a)) & 0x1fffff) - 1048576;
              near = near && std::llabs(rc_a - cell[a]) <= reach;
            }
            if (!near) continue;
            const double dx = q[0] - rows[3 * j], dy = q[1] - rows[3 * j + 1], dz = q[2] - rows[3 * j + 2];
            const double d2 = dx * dx + (dy * dy + dz * dz);
            if (d2 < want_d2[i] || (d2 == want_d2[i] && want_row[i] < 0)) {  // (j ascends: an equal d2 later does not win)
              want_d2[i] = d2;
              want_row[i] = static_cast<int32_t>(j);
            }
          }
          if (want_row[i] >= 0) {
            ++want_counts[1];
            if (want_d2[i] <= md2) ++want_counts[2];
          }
        }
        for (int subset = 0; subset < 32; ++subset) {  // every subset of the five per-point buffers, each of exactly n entries
          const bool w_row = subset & 1, w_d2 = subset & 2, w_key = subset & 4, w_attr = (subset & 8) && with_attr, w_ev = (subset & 16) && with_ev;
          int32_t* o_row = w_row ? exactly<int32_t>(n) : nullptr;
          double* o_d2 = w_d2 ? exactly<double>(n) : nullptr;
          uint64_t* o_key = w_key ? exactly<uint64_t>(n) : nullptr;
          uint32_t* o_attr = w_attr ? exactly<uint32_t>(n) : nullptr;
          uint32_t* o_ev = w_ev ? exactly<uint32_t>(n) : nullptr;
          uint64_t counts[3] = {7, 7, 7};
          const bool any = w_row || w_d2 || w_key || w_attr || w_ev;
          if (any && n > 0) {  // too short by one: refused, nothing written (the buffers would not survive a write of n entries either)
            if (madicp_host_map_query(map, cloud, n, QR, Qt, reach, max_dist, o_row, o_d2, o_key, o_attr, o_ev, n - 1, counts) != MADICP_ERR_CAPACITY ||
                counts[0] != 7)
              return fail("a short buffer", set, n);
          }
          rc = madicp_host_map_query(map, cloud, n, QR, Qt, reach, max_dist, o_row, o_d2, o_key, o_attr, o_ev, any ? n : 0, counts);
          if (rc != MADICP_OK) return fail("query", set, rc);
          if (std::memcmp(counts, want_counts, sizeof(counts)) != 0) return fail("counts", set, n);
          for (int64_t i = 0; i < n; ++i) {
            const int32_t r = want_row[i];
            if (w_row && o_row[i] != r) return fail("row", set, i);
            if (w_d2 && std::memcmp(&o_d2[i], &want_d2[i], sizeof(double)) != 0) return fail("d2", set, i);
            if (w_key && o_key[i] != (r >= 0 ? keys[r] : kExportNoKey)) return fail("key", set, i);
            if (w_attr && o_attr[i] != (r >= 0 ? attr[r] : 0u)) return fail("attr", set, i);
            if (w_ev && o_ev[i] != (r >= 0 ? ev[r] : 0u)) return fail("ev", set, i);
          }
          std::free(o_row);
          std::free(o_d2);
          std::free(o_key);
          std::free(o_attr);
          std::free(o_ev);
        }
        // a column the map lacks, a reach and a max_dist outside the rule: refused, nothing written
        uint32_t probe = 7;
        uint64_t counts[3] = {7, 7, 7};
        if (!with_attr && madicp_host_map_query(map, cloud, n, QR, Qt, reach, 1.0, nullptr, nullptr, nullptr, &probe, nullptr, n, counts) != MADICP_ERR_INVALID)
          return fail("out_attr without the column", set, n);
        if (!with_ev && madicp_host_map_query(map, cloud, n, QR, Qt, reach, 1.0, nullptr, nullptr, nullptr, nullptr, &probe, n, counts) != MADICP_ERR_INVALID)
          return fail("out_ev without the column", set, n);
        if (madicp_host_map_query(map, cloud, n, QR, Qt, 2, 1.0, nullptr, nullptr, nullptr, nullptr, nullptr, n, counts) != MADICP_ERR_INVALID ||
            madicp_host_map_query(map, cloud, n, QR, Qt, reach, -1.0, nullptr, nullptr, nullptr, nullptr, nullptr, n, counts) != MADICP_ERR_INVALID ||
            madicp_host_map_query(map, cloud, n, QR, Qt, reach, std::nan(""), nullptr, nullptr, nullptr, nullptr, nullptr, n, counts) != MADICP_ERR_INVALID)
          return fail("reach and max_dist", set, n);
        if (probe != 7 || counts[0] != 7 || counts[1] != 7 || counts[2] != 7) return fail("a refusal wrote", set, n);
      }
      std::free(cloud);
    }
    std::free(rows);
    std::free(keys);
    std::free(attr);
    std::free(ev);
    madicp_host_map_destroy(map);
    ++sets;
  }
  std::printf("%d sets clean\n", sets);
  return 0;
}
