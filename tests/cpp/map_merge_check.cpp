// Stand-alone check of the host voxel map's merge of saved rows (madicp_host_map_merge_rows: csrc/host/voxel_map.cpp + voxel_map.h,
// the rule of csrc/common/map_merge.h) under AddressSanitizer and UndefinedBehaviorSanitizer: compiled and run by
// tests/test_map_merge_sanitized.py.  Every column of a batch lives in a heap buffer of EXACTLY n entries (n keys, 3 n floats, n
// words, n evidence words, 10 n moment words): a read past any of them ends the program with the sanitizer's report.  After every
// merge every column the map hands out is held to a restatement kept in this program — ordered containers and 128-bit sums, nothing
// shared with the code under test.  Maps of all six kinds, batch sizes around 64 and 1024, repeated keys, growth from
// initial_rows = 1, a fold between two merges, and refusals that must leave the map and both answers as they were.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "madicp_host.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int fail(const char* what, int set, long long i) {
  std::fprintf(stderr, "set %d step %lld: %s\n", set, i, what);
  return 1;
}

template <class T>
static T* exactly(int64_t n) {  // (a zero-byte block is legal, and every access to it is out of bounds)
  return static_cast<T*>(std::malloc(sizeof(T) * static_cast<size_t>(n)));
}

struct Kind {
  bool attr, ev, mom;
};
constexpr uint32_t kCap = 6, kMaxCount = 4;
constexpr double kVoxel = 0.25;

// the restatement: the map as rows in order, and the index of a key
struct Row {
  uint64_t key;
  uint32_t xyz[3], attr;
  unsigned __int128 ev;
  unsigned __int128 mom[10];
};
struct Model {
  std::vector<Row> rows;
  std::map<uint64_t, size_t> at;
};

struct Batch {
  int64_t n;
  uint64_t* keys;
  float* xyz;
  uint32_t *attr, *ev;
  uint64_t* mom;
  void release() {
    std::free(keys), std::free(xyz), std::free(attr), std::free(ev), std::free(mom);
  }
};

static Batch make_batch(const Kind& k, int64_t n, int64_t pool, uint32_t& seed) {
  Batch b{n, exactly<uint64_t>(n), exactly<float>(3 * n), k.attr ? exactly<uint32_t>(n) : nullptr, k.ev ? exactly<uint32_t>(n) : nullptr,
          k.mom ? exactly<uint64_t>(10 * n) : nullptr};
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t c = lcg(seed) % static_cast<uint32_t>(pool);  // (a cell index: repeats where pool < n)
    b.keys[i] = (c * 2654435761ull) & 0x7fffffffffffffffull;
    for (int a = 0; a < 3; ++a) {
      const uint32_t bits = lcg(seed) | (i % 7 == 0 ? 0x7f800000u : 0u);  // (every seventh row: NaN or inf bits)
      std::memcpy(&b.xyz[3 * i + a], &bits, 4);
    }
    if (b.attr) b.attr[i] = lcg(seed);
    if (b.ev) b.ev[i] = 1 + lcg(seed) % 3;
    if (b.mom) {
      const uint64_t cnt = 1 + lcg(seed) % 3, w[3] = {lcg(seed) % 65536, lcg(seed) % 65536, lcg(seed) % 65536};
      const uint64_t one[10] = {1, w[0], w[1], w[2], w[0] * w[0], w[0] * w[1], w[0] * w[2], w[1] * w[1], w[1] * w[2], w[2] * w[2]};
      for (int q = 0; q < 10; ++q) b.mom[10 * i + q] = cnt * one[q];
    }
  }
  return b;
}

static void restate(Model& M, const Kind& k, const Batch& b) {
  std::vector<unsigned __int128> before(M.rows.size());
  for (size_t r = 0; r < M.rows.size(); ++r) before[r] = M.rows[r].mom[0];
  for (int64_t i = 0; i < b.n; ++i) {  // rows first: the lowest index of every key the map lacks, in ascending order
    if (M.at.count(b.keys[i])) continue;
    Row r{};
    r.key = b.keys[i];
    std::memcpy(r.xyz, b.xyz + 3 * i, 12);
    r.attr = k.attr ? b.attr[i] : 0;
    M.at[r.key] = M.rows.size();
    M.rows.push_back(r);
    before.push_back(0);
  }
  for (int64_t i = 0; i < b.n; ++i) {
    Row& r = M.rows[M.at[b.keys[i]]];
    if (k.ev) r.ev += b.ev[i];
    if (k.mom && before[M.at[b.keys[i]]] < kMaxCount)
      for (int q = 0; q < 10; ++q) r.mom[q] += b.mom[10 * i + q];
  }
  if (k.ev)
    for (Row& r : M.rows)
      if (r.ev > kCap) r.ev = kCap;
}

static int compare(madicp_host_map* map, const Model& M, const Kind& k, int set, long long step) {
  int64_t rows = -1, got = -1;
  if (madicp_host_map_size(map, &rows) != MADICP_OK || rows != static_cast<int64_t>(M.rows.size())) return fail("size", set, step);
  float* xyz = exactly<float>(3 * rows);
  uint64_t* keys = exactly<uint64_t>(rows);
  uint32_t* attr = k.attr ? exactly<uint32_t>(rows) : nullptr;
  if (madicp_host_map_download_rows(map, 0, xyz, keys, attr, rows, &got) != MADICP_OK || got != rows) return fail("download_rows", set, step);
  uint32_t* ev = k.ev ? exactly<uint32_t>(rows) : nullptr;
  if (k.ev && madicp_host_map_download_evidence(map, 0, ev, rows, &got) != MADICP_OK) return fail("download_evidence", set, step);
  uint64_t* mom = k.mom ? exactly<uint64_t>(10 * rows) : nullptr;
  if (k.mom && madicp_host_map_download_moments(map, 0, mom, rows, &got) != MADICP_OK) return fail("download_moments", set, step);
  for (int64_t r = 0; r < rows; ++r) {
    const Row& w = M.rows[r];
    if (keys[r] != w.key) return fail("a key or the row order", set, r);
    if (std::memcmp(xyz + 3 * r, w.xyz, 12) != 0) return fail("a row's float bits", set, r);
    if (k.attr && attr[r] != w.attr) return fail("an attribute word", set, r);
    if (k.ev && ev[r] != static_cast<uint32_t>(w.ev)) return fail("an evidence word", set, r);
    for (int q = 0; k.mom && q < 10; ++q)
      if (mom[10 * r + q] != static_cast<uint64_t>(w.mom[q]) || (w.mom[q] >> 64) != 0) return fail("a moment word", set, r);
  }
  std::free(xyz), std::free(keys), std::free(attr), std::free(ev), std::free(mom);
  return 0;
}

// the model of a map that folds made, read off its downloads (the restatement of a FOLD is not this program's business)
static int adopt(madicp_host_map* map, Model& M, const Kind& k, int set) {
  int64_t rows = 0, got = 0;
  madicp_host_map_size(map, &rows);
  float* xyz = exactly<float>(3 * rows);
  uint64_t* keys = exactly<uint64_t>(rows);
  uint32_t* attr = k.attr ? exactly<uint32_t>(rows) : nullptr;
  uint32_t* ev = k.ev ? exactly<uint32_t>(rows) : nullptr;
  uint64_t* mom = k.mom ? exactly<uint64_t>(10 * rows) : nullptr;
  if (madicp_host_map_download_rows(map, 0, xyz, keys, attr, rows, &got) != MADICP_OK) return fail("adopt", set, 0);
  if (k.ev && madicp_host_map_download_evidence(map, 0, ev, rows, &got) != MADICP_OK) return fail("adopt", set, 1);
  if (k.mom && madicp_host_map_download_moments(map, 0, mom, rows, &got) != MADICP_OK) return fail("adopt", set, 2);
  M = Model{};
  for (int64_t r = 0; r < rows; ++r) {
    Row w{};
    w.key = keys[r];
    std::memcpy(w.xyz, xyz + 3 * r, 12);
    w.attr = k.attr ? attr[r] : 0;
    w.ev = k.ev ? ev[r] : 0;
    for (int q = 0; k.mom && q < 10; ++q) w.mom[q] = mom[10 * r + q];
    M.at[w.key] = M.rows.size();
    M.rows.push_back(w);
  }
  std::free(xyz), std::free(keys), std::free(attr), std::free(ev), std::free(mom);
  return 0;
}

static int refusals(madicp_host_map* map, const Model& M, const Kind& k, int set, uint32_t& seed) {
  int step = 0;
  auto refused = [&](const Batch& b, double voxel, int64_t n, int code, const char* what) {
    int64_t added = -7, rows = -7;
    ++step;
    const int rc = madicp_host_map_merge_rows(map, voxel, b.keys, b.xyz, b.attr, b.ev, b.mom, n, &added, &rows);
    if (rc != code || added != -7 || rows != -7) return fail(what, set, step);
    return compare(map, M, k, set, step);
  };
  Batch b = make_batch(k, 5, 1000, seed);
  if (refused(b, 0.5, 5, MADICP_ERR_INVALID, "another voxel")) return 1;
  if (refused(b, kVoxel, -1, MADICP_ERR_INVALID, "n < 0")) return 1;
  int64_t added = -7;
  if (madicp_host_map_merge_rows(map, kVoxel, b.keys, b.xyz, b.attr, b.ev, b.mom, 5, nullptr, &added) != MADICP_ERR_INVALID || added != -7)
    return fail("null out_added", set, step);
  if (madicp_host_map_merge_rows(nullptr, kVoxel, b.keys, b.xyz, b.attr, b.ev, b.mom, 5, &added, &added) != MADICP_ERR_INVALID || added != -7)
    return fail("null map", set, step);
  b.keys[4] |= 1ull << 63;
  if (refused(b, kVoxel, 5, MADICP_ERR_INVALID, "bit 63")) return 1;
  b.keys[4] &= ~(1ull << 63);
  {
    Batch c = b;
    c.xyz = nullptr;
    if (refused(c, kVoxel, 5, MADICP_ERR_INVALID, "null rows")) return 1;
    uint32_t* extra = exactly<uint32_t>(5);
    uint64_t* extra_mom = exactly<uint64_t>(50);
    for (int i = 0; i < 5; ++i) extra[i] = 1;
    for (int i = 0; i < 50; ++i) extra_mom[i] = 1;
    c = b;
    if (k.attr) c.attr = nullptr; else c.attr = extra;
    if (refused(c, kVoxel, 5, MADICP_ERR_INVALID, "the attribute column missing or surplus")) return 1;
    c = b;
    if (k.ev) c.ev = nullptr; else c.ev = extra;
    if (refused(c, kVoxel, 5, MADICP_ERR_INVALID, "the evidence column missing or surplus")) return 1;
    c = b;
    if (k.mom) c.mom = nullptr; else c.mom = extra_mom;
    if (refused(c, kVoxel, 5, MADICP_ERR_INVALID, "the moments missing or surplus")) return 1;
    std::free(extra), std::free(extra_mom);
  }
  if (k.ev) {
    const uint32_t keep = b.ev[2];
    for (uint32_t bad : {0u, 0x80000000u, 0xffffffffu}) {
      b.ev[2] = bad;
      if (refused(b, kVoxel, 5, MADICP_ERR_INVALID, "evidence outside 1 .. 2^31 - 1")) return 1;
    }
    b.ev[2] = keep;
  }
  if (k.mom) {
    uint64_t keep[10];
    std::memcpy(keep, b.mom + 30, sizeof(keep));
    const uint64_t cnt = keep[0];
    const struct { int at; uint64_t value; } bad[] = {{0, 0}, {0, 1ull << 31}, {0, ~0ull}, {1, 65535 * cnt + 1}, {3, ~0ull},
                                                      {4, 65535ull * 65535ull * cnt + 1}, {9, ~0ull}};
    for (const auto& c : bad) {
      b.mom[30 + c.at] = c.value;
      if (refused(b, kVoxel, 5, MADICP_ERR_INVALID, "a moment word out of its bound")) return 1;
      std::memcpy(b.mom + 30, keep, sizeof(keep));
    }
    uint64_t all[50];
    std::memcpy(all, b.mom, sizeof(all));
    for (int i = 0; i < 50; ++i) b.mom[i] = 0;
    for (int i = 0; i < 5; ++i) b.mom[10 * i] = i == 0 ? 0x7ffffffbull : 1;  // each legal, together 2^31 - 1 ... and one more
    b.mom[10] = 2;
    if (refused(b, kVoxel, 5, MADICP_ERR_INVALID, "counts that sum past 2^31 - 1")) return 1;
    std::memcpy(b.mom, all, sizeof(all));
  }
  b.release();
  return 0;
}

int main() {
  const double kI[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kZ[3] = {0, 0, 0};
  const Kind kinds[6] = {{false, false, false}, {true, false, false}, {false, true, false}, {true, true, false}, {false, true, true}, {true, true, true}};
  const int64_t sizes[] = {0, 1, 63, 64, 65, 1023, 1024, 1025};
  int sets = 0;
  for (int set = 0; set < 48; ++set) {
    uint32_t seed = 9000u + set;
    const Kind k = kinds[set % 6];
    const uint32_t evidence[3] = {2, 1, kCap};
    const int64_t max_rows = 1 << 20;
    madicp_host_map* map = nullptr;
    const int rc = k.mom  ? madicp_host_map_create_mom(kVoxel, 1, max_rows, k.attr, evidence, kMaxCount, &map)
                   : k.ev ? madicp_host_map_create_ev(kVoxel, 1, max_rows, k.attr, 2, 1, kCap, &map)
                          : (k.attr ? madicp_host_map_create_attr(kVoxel, 1, max_rows, &map) : madicp_host_map_create(kVoxel, 1, max_rows, &map));
    if (rc != MADICP_OK) return fail("create", set, rc);
    Model M;
    const int64_t n = sizes[set % 8];
    for (int step = 0; step < 3; ++step) {
      // step 0: many repeats; 1: half the pool is new; 2: all entries on ONE key (sets 5, 13, ...) or few repeats
      const int64_t pool = step == 0 ? n / 2 + 1 : step == 1 ? n + 1 : (set % 8 == 5 ? 1 : 4 * n + 1);
      Batch b = make_batch(k, n, pool, seed);
      const size_t before = M.rows.size();
      restate(M, k, b);
      int64_t added = -1, rows = -1;
      if (madicp_host_map_merge_rows(map, kVoxel, b.keys, b.xyz, b.attr, b.ev, b.mom, n, &added, &rows) != MADICP_OK) return fail("merge", set, step);
      b.release();
      if (rows != static_cast<int64_t>(M.rows.size())) return fail("out_rows", set, step);
      if (added != static_cast<int64_t>(M.rows.size() - before)) return fail("out_added", set, step);
      if (compare(map, M, k, set, step)) return 1;
      if (step == 0) {  // a fold between two merges: it goes on from the merged rows, and the next merge from what it left
        double* pts = exactly<double>(3 * 40);
        for (int i = 0; i < 120; ++i) pts[i] = ((lcg(seed) >> 8) / 16777216.0 - 0.5) * 3.0;
        int64_t a = 0, r = 0;
        if (madicp_host_map_insert(map, pts, 40, kI, kZ, &a, &r) != MADICP_OK) return fail("fold", set, step);
        std::free(pts);
        if (adopt(map, M, k, set)) return 1;
      }
    }
    int64_t none = -1, held = -1;
    if (madicp_host_map_merge_rows(map, kVoxel, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &none, &held) != MADICP_OK || none != 0 ||
        held != static_cast<int64_t>(M.rows.size()))
      return fail("n = 0 with null columns is legal and does nothing", set, 0);
    if (refusals(map, M, k, set, seed)) return 1;
    madicp_host_map_destroy(map);
    ++sets;
  }
  std::printf("%d sets clean\n", sets);
  return 0;
}
