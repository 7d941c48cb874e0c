// Stand-alone check of the host voxel map's evidence column (madicp_host_map_create_ev / _download_evidence /
// _download_min_evidence: csrc/host/voxel_map.cpp + voxel_map.h) under AddressSanitizer and UndefinedBehaviorSanitizer: compiled
// and run by tests/test_map_evidence_sanitized.py.  Every cloud lives in a heap buffer of EXACTLY n rows and every download goes
// into buffers of EXACTLY the reported size: a write past the last row ends the program with the sanitizer's report.  The results
// are held to the obvious reading of the rule on a lattice where it can be read off without a ray walk: voxel 1, every point at
// a cell centre, and clearings whose rays run along +x from a cell centre — the ray to the centre k cells on traverses exactly
// the cells 1 .. k on its way (sample k' sits k' cells on) and occupies cell k.
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
  uint32_t e, word;
  uint64_t key() const {
    return static_cast<uint64_t>(c[0] + 1048576) | static_cast<uint64_t>(c[1] + 1048576) << 21 | static_cast<uint64_t>(c[2] + 1048576) << 42;
  }
};

template <class T>
static T* exactly(int64_t n) {  // (a zero-byte block is legal, and every write to it is out of bounds)
  return static_cast<T*>(std::malloc(sizeof(T) * static_cast<size_t>(n)));
}

static const double kR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kT[3] = {0, 0, 0};

// the map's columns into buffers of exactly its size, and the filtered download at min_e into buffers of exactly ITS size
static bool same_map(madicp_host_map* map, bool with_attr, const std::vector<Row>& want, uint32_t min_e) {
  int64_t m = -7, got = -7;
  if (madicp_host_map_size(map, &m) != MADICP_OK || m != static_cast<int64_t>(want.size())) return false;
  uint32_t* ev = exactly<uint32_t>(m);
  uint64_t* keys = exactly<uint64_t>(m);
  bool ok = madicp_host_map_download_evidence(map, 0, ev, m, &got) == MADICP_OK && got == m;
  ok = ok && madicp_host_map_download_keys(map, 0, keys, m, &got) == MADICP_OK && got == m;
  for (int64_t j = 0; ok && j < m; ++j) ok = ev[j] == want[j].e && keys[j] == want[j].key();
  if (ok && m > 1) {  // a window that starts inside the map, and one that is too short by one
    ok = madicp_host_map_download_evidence(map, m - 1, ev, 1, &got) == MADICP_OK && got == 1 && ev[0] == want.back().e;
    ok = ok && madicp_host_map_download_evidence(map, 0, ev, m - 1, &got) == MADICP_ERR_CAPACITY && got == m;
  }
  std::free(ev);
  std::free(keys);
  if (!ok) return false;
  std::vector<Row> sel;
  for (const Row& r : want)
    if (r.e >= min_e) sel.push_back(r);
  const int64_t n = static_cast<int64_t>(sel.size());
  float probe[3];
  if (n > 0) {  // the count first, from a buffer too short by one: nothing written
    float* shorter = exactly<float>(3 * (n - 1));
    ok = madicp_host_map_download_min_evidence(map, min_e, shorter, nullptr, nullptr, nullptr, n - 1, &got) == MADICP_ERR_CAPACITY && got == n;
    std::free(shorter);
  } else {
    ok = madicp_host_map_download_min_evidence(map, min_e, probe, nullptr, nullptr, nullptr, 0, &got) == MADICP_OK && got == 0;
  }
  if (!ok) return false;
  float* rows = exactly<float>(3 * n);
  uint64_t* k2 = exactly<uint64_t>(n);
  uint32_t* words = with_attr ? exactly<uint32_t>(n) : nullptr;
  uint32_t* e2 = exactly<uint32_t>(n);
  ok = madicp_host_map_download_min_evidence(map, min_e, n ? rows : probe, k2, words, e2, n, &got) == MADICP_OK && got == n;
  for (int64_t j = 0; ok && j < n; ++j) {
    for (int a = 0; a < 3; ++a) ok = ok && rows[3 * j + a] == static_cast<float>(sel[j].c[a] + 0.5);
    ok = ok && k2[j] == sel[j].key() && e2[j] == sel[j].e && (!words || words[j] == sel[j].word);
  }
  std::free(rows);
  std::free(k2);
  std::free(words);
  std::free(e2);
  return ok;
}

int main() {
  int sets = 0;
  for (int set = 0; set < 48; ++set) {
    uint32_t seed = 977u * static_cast<uint32_t>(set) + 5u;
    const bool with_attr = set % 2 == 1;
    const uint32_t hit = 1 + (lcg(seed) >> 8) % 3, miss = 1 + (lcg(seed) >> 8) % 3, cap = hit + (lcg(seed) >> 8) % 6;
    madicp_host_map* map = nullptr;
    if (madicp_host_map_create_ev(1.0, set % 3 == 0 ? 1 : 64, 1 << 20, with_attr ? 1 : 0, hit, miss, cap, &map) != MADICP_OK)
      return fail("create", set, 0);
    if (set % 4 == 0 && madicp_host_map_track_removed(map, 1) != MADICP_OK) return fail("track", set, 0);
    std::vector<Row> want;
    const int nx = 6 + set % 19, ny = 1 + set % 3;
    for (long long step = 0; step < 24; ++step) {
      const uint32_t kind = (lcg(seed) >> 8) % 3;
      if (kind != 2 || want.empty()) {  // a fold of n random cell centres, repeats among them
        const int64_t n = 1 + (lcg(seed) >> 8) % (set % 5 == 0 ? 700 : 40);
        double* xyz = exactly<double>(3 * n);
        uint32_t* attr = exactly<uint32_t>(n);
        std::set<uint64_t> met;
        const size_t before = want.size();
        for (int64_t i = 0; i < n; ++i) {
          Row r{{static_cast<int>((lcg(seed) >> 8) % static_cast<uint32_t>(nx)), static_cast<int>((lcg(seed) >> 8) % static_cast<uint32_t>(ny)), 0},
                hit, static_cast<uint32_t>(1000 * step + i)};
          for (int a = 0; a < 3; ++a) xyz[3 * i + a] = r.c[a] + 0.5;
          attr[i] = r.word;
          bool found = false;
          for (size_t j = 0; j < want.size() && !found; ++j)
            if (want[j].key() == r.key()) {
              found = true;
              if (j < before && met.insert(r.key()).second) want[j].e = want[j].e + hit < cap ? want[j].e + hit : cap;
            }
          if (!found) want.push_back(r);
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
            if (r.e <= miss) continue;
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
      if (!same_map(map, with_attr, want, 1 + static_cast<uint32_t>(step) % (cap + 1))) return fail("columns", set, step);
    }
    if (!same_map(map, with_attr, want, 0) || !same_map(map, with_attr, want, cap + 1)) return fail("thresholds", set, 24);
    madicp_host_map_destroy(map);
    ++sets;
  }
  std::printf("%d sets clean\n", sets);
  return 0;
}
