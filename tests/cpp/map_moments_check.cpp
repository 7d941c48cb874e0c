// Stand-alone check of the host voxel map's moments (madicp_host_map_create_mom / _download_moments / _download_surfels:
// csrc/host/voxel_map.cpp + voxel_map.h, the rule of csrc/common/voxel_moments.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer: compiled and run by tests/test_map_moments_sanitized.py.  Every cloud lives in a heap buffer of
// EXACTLY n rows and every download goes into buffers of EXACTLY the reported size: a write past the last row ends the program with
// the sanitizer's report.  The results are held to the obvious reading of the rule on a lattice where it can be read off: voxel 1,
// every point a quarter, a half or three quarters into its cell on every axis (offsets 16384, 32768, 49152 exactly), and clearings
// whose rays run along +x from a cell centre — the ray to the centre k cells on traverses exactly the cells 1 .. k and occupies
// cell k.  Odd sets carry the evidence column as well, every fourth the removal log, every third grows from one row.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "madicp_host.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int fail(const char* what, int set, long long i) {
  std::fprintf(stderr, "set %d step %lld: %s\n", set, i, what);
  return 1;
}

struct Row {
  int c[3];
  uint32_t e;
  uint64_t m[10];
  uint64_t key() const {
    return static_cast<uint64_t>(c[0] + 1048576) | static_cast<uint64_t>(c[1] + 1048576) << 21 | static_cast<uint64_t>(c[2] + 1048576) << 42;
  }
  void take(const uint32_t* w) {
    m[0] += 1;
    for (int a = 0; a < 3; ++a) m[1 + a] += w[a];
    int j = 4;
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) m[j++] += static_cast<uint64_t>(w[a]) * w[b];
  }
};

template <class T>
static T* exactly(int64_t n) {  // (a zero-byte block is legal, and every write to it is out of bounds)
  return static_cast<T*>(std::malloc(sizeof(T) * static_cast<size_t>(n)));
}

static const double kR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kT[3] = {0, 0, 0};

// the window [first, size) of the map's moments and surfels into buffers of exactly its size
static bool same_window(madicp_host_map* map, const std::vector<Row>& want, int64_t first, bool all_columns) {
  const int64_t m = static_cast<int64_t>(want.size()) - first;
  int64_t got = -7;
  uint64_t* mom = exactly<uint64_t>(10 * m);
  uint64_t probe_m[10];
  bool ok = madicp_host_map_download_moments(map, first, m ? mom : probe_m, m, &got) == MADICP_OK && got == m;
  for (int64_t j = 0; ok && j < m; ++j) ok = std::memcmp(mom + 10 * j, want[first + j].m, sizeof(uint64_t) * 10) == 0;
  std::free(mom);
  if (!ok) return false;
  float* cen = exactly<float>(3 * m);
  float* nrm = all_columns ? exactly<float>(3 * m) : nullptr;
  float* eig = all_columns ? exactly<float>(3 * m) : nullptr;
  uint32_t* cnt = exactly<uint32_t>(m);
  float probe[3];
  ok = madicp_host_map_download_surfels(map, first, m ? cen : probe, nrm, eig, cnt, m, &got) == MADICP_OK && got == m;
  for (int64_t j = 0; ok && j < m; ++j) {
    const Row& r = want[first + j];
    ok = cnt[j] == r.m[0];
    for (int a = 0; ok && a < 3; ++a) {
      const double mean = static_cast<double>(r.m[1 + a]) / static_cast<double>(r.m[0]);
      ok = cen[3 * j + a] == static_cast<float>((static_cast<double>(r.c[a]) + (mean + 0.5) / 65536.0) * 1.0);
      if (ok && all_columns) {
        ok = std::isfinite(nrm[3 * j + a]) && std::isfinite(eig[3 * j + a]) && (r.m[0] >= 3 || nrm[3 * j + a] == 0.0f);
        ok = ok && eig[3 * j + a] > -1e-6f && eig[3 * j + a] < 0.2f;  // (offsets within half a cell of each other: a variance of at most 1/16 per axis)
      }
    }
  }
  if (ok && m > 0) {  // too short by one: the count, nothing written
    ok = madicp_host_map_download_surfels(map, first, probe, nullptr, nullptr, nullptr, m - 1, &got) == MADICP_ERR_CAPACITY && got == m;
    ok = ok && madicp_host_map_download_moments(map, first, probe_m, m - 1, &got) == MADICP_ERR_CAPACITY && got == m;
  }
  std::free(cen);
  std::free(nrm);
  std::free(eig);
  std::free(cnt);
  return ok;
}

static bool same_map(madicp_host_map* map, bool with_ev, const std::vector<Row>& want, long long step) {
  int64_t m = -7, got = -7;
  if (madicp_host_map_size(map, &m) != MADICP_OK || m != static_cast<int64_t>(want.size())) return false;
  uint64_t* keys = exactly<uint64_t>(m);
  uint32_t* ev = with_ev ? exactly<uint32_t>(m) : nullptr;
  uint64_t probe_k[1];
  uint32_t probe_e[1];
  bool ok = madicp_host_map_download_keys(map, 0, m ? keys : probe_k, m, &got) == MADICP_OK && got == m;
  if (with_ev) ok = ok && madicp_host_map_download_evidence(map, 0, m ? ev : probe_e, m, &got) == MADICP_OK && got == m;
  for (int64_t j = 0; ok && j < m; ++j) ok = keys[j] == want[j].key() && (!with_ev || ev[j] == want[j].e);
  std::free(keys);
  std::free(ev);
  return ok && same_window(map, want, 0, step % 2 == 0) && same_window(map, want, m / 2, step % 2 == 1) && same_window(map, want, m, true);
}

int main() {
  int sets = 0;
  for (int set = 0; set < 48; ++set) {
    uint32_t seed = 991u * static_cast<uint32_t>(set) + 3u;
    const bool with_attr = set % 4 >= 2, with_ev = set % 2 == 1;
    const uint32_t hit = 1 + (lcg(seed) >> 8) % 3, miss = 1 + (lcg(seed) >> 8) % 3, cap = hit + (lcg(seed) >> 8) % 6;
    const uint32_t evidence[3] = {hit, miss, cap};
    const uint32_t max_count = set % 6 == 5 ? 0x80000000u : 1 + (lcg(seed) >> 8) % 9;
    madicp_host_map* map = nullptr;
    if (madicp_host_map_create_mom(1.0, set % 3 == 0 ? 1 : 64, 1 << 20, with_attr ? 1 : 0, with_ev ? evidence : nullptr, max_count, &map) !=
        MADICP_OK)
      return fail("create", set, 0);
    if (set % 4 == 0 && madicp_host_map_track_removed(map, 1) != MADICP_OK) return fail("track", set, 0);
    std::vector<Row> want;
    const int nx = 6 + set % 19, ny = 1 + set % 3;
    for (long long step = 0; step < 24; ++step) {
      const uint32_t kind = (lcg(seed) >> 8) % 3;
      if (kind != 2 || want.empty()) {  // a fold of n random points, repeats among their cells
        const int64_t n = 1 + (lcg(seed) >> 8) % (set % 5 == 0 ? 700 : 40);
        double* xyz = exactly<double>(3 * n);
        uint32_t* attr = exactly<uint32_t>(n);
        std::set<uint64_t> met;
        const size_t before = want.size();
        std::vector<uint64_t> n_before;
        for (const Row& r : want) n_before.push_back(r.m[0]);
        for (int64_t i = 0; i < n; ++i) {
          Row r{{static_cast<int>((lcg(seed) >> 8) % static_cast<uint32_t>(nx)), static_cast<int>((lcg(seed) >> 8) % static_cast<uint32_t>(ny)), 0},
                hit, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
          uint32_t w[3];
          for (int a = 0; a < 3; ++a) {
            const uint32_t quarter = 1 + (lcg(seed) >> 8) % 3;
            w[a] = 16384u * quarter;
            xyz[3 * i + a] = r.c[a] + 0.25 * quarter;
          }
          attr[i] = static_cast<uint32_t>(1000 * step + i);
          size_t at = want.size();
          for (size_t j = 0; j < want.size() && at == want.size(); ++j)
            if (want[j].key() == r.key()) at = j;
          if (at == want.size()) {
            want.push_back(r);
            n_before.push_back(0);
          } else if (at < before && met.insert(r.key()).second) {
            want[at].e = want[at].e + hit < cap ? want[at].e + hit : cap;
          }
          if (n_before[at] < max_count) want[at].take(w);
        }
        int64_t added = -7, rows = -7;
        const int rc = with_attr ? madicp_host_map_insert_attr(map, xyz, attr, n, kR, kT, &added, &rows)
                                 : madicp_host_map_insert(map, xyz, n, kR, kT, &added, &rows);
        std::free(xyz);
        std::free(attr);
        if (rc != MADICP_OK || rows != static_cast<int64_t>(want.size()) || added != static_cast<int64_t>(want.size() - before))
          return fail("fold", set, step);
      } else {  // a clearing: rays along +x from the centre of cell (ox, oy) to the centres k cells on
        const int ox = static_cast<int>((lcg(seed) >> 8) % static_cast<uint32_t>(nx)), oy = static_cast<int>((lcg(seed) >> 8) % static_cast<uint32_t>(ny));
        const int64_t n = 1 + (lcg(seed) >> 8) % 3;
        double* xyz = exactly<double>(3 * n);
        std::set<int> traversed, occupied;
        for (int64_t i = 0; i < n; ++i) {
          const int k = static_cast<int>((lcg(seed) >> 8) % static_cast<uint32_t>(nx));
          xyz[3 * i] = ox + k + 0.5;
          xyz[3 * i + 1] = oy + 0.5;
          xyz[3 * i + 2] = 0.5;
          occupied.insert(ox + k);
          for (int s = 1; s <= k; ++s) traversed.insert(ox + s);
        }
        const double origin[3] = {ox + 0.5, oy + 0.5, 0.5};
        const int64_t watermark = static_cast<int64_t>(want.size() / 2);
        std::vector<Row> kept;
        int64_t mark = 0;
        for (size_t j = 0; j < want.size(); ++j) {
          Row r = want[j];
          const bool missed = r.c[1] == oy && traversed.count(r.c[0]) && !occupied.count(r.c[0]);
          if (missed) {
            if (!with_ev || r.e <= miss) continue;
            r.e -= miss;
          }
          kept.push_back(r);
          if (static_cast<int64_t>(j) < watermark) ++mark;
        }
        int64_t removed = -7, rows = -7, out_mark = -7;
        const int rc = madicp_host_map_clear_rays(map, xyz, n, kR, kT, origin, 0.0, watermark, &removed, &rows, &out_mark);
        std::free(xyz);
        if (rc != MADICP_OK || rows != static_cast<int64_t>(kept.size()) || removed != static_cast<int64_t>(want.size() - kept.size()) ||
            out_mark != mark)
          return fail("clear", set, step);
        want.swap(kept);
      }
      if (!same_map(map, with_ev, want, step)) return fail("columns", set, step);
    }
    if (madicp_host_map_clear(map) != MADICP_OK || !same_map(map, with_ev, std::vector<Row>(), 0)) return fail("clear", set, 24);
    madicp_host_map_destroy(map);
    ++sets;
  }
  std::printf("%d sets clean\n", sets);
  return 0;
}
