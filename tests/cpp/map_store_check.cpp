// Stand-alone check of HostMapStore (csrc/host/map_store.h) — compiled and run by tests/test_map_store.py, plain and under
// AddressSanitizer + UndefinedBehaviorSanitizer.  One scripted sequence is driven through a HostMapStore and, beside it, through a
// VoxelMap called directly with the same arguments, for all eight combinations of attribute, evidence and moments: every return code
// and every output byte must be equal.  Every cloud lives in a heap buffer of EXACTLY n rows and every output goes into a buffer of
// EXACTLY the entries it may hold, pre-filled with the same pattern on both sides: a write past the end ends the program with the
// sanitizer's report, and a buffer one side leaves alone must be left alone by the other.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "map_store.h"

using namespace madicp_host;

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t& s) { return (double)(lcg(s) >> 8) / 16777216.0; }  // [0, 1)

// a heap block of exactly n entries, every byte 0xA5 (a zero-byte block is legal, and every write to it is out of bounds)
template <class T>
struct Exactly {
  T* p;
  size_t bytes;
  explicit Exactly(int64_t n) : p(static_cast<T*>(std::malloc(sizeof(T) * static_cast<size_t>(n)))), bytes(sizeof(T) * static_cast<size_t>(n)) {
    if (bytes) std::memset(p, 0xA5, bytes);
  }
  ~Exactly() { std::free(p); }
  Exactly(const Exactly&) = delete;
  bool same(const Exactly& o) const { return bytes == o.bytes && (bytes == 0 || std::memcmp(p, o.p, bytes) == 0); }
};

struct Cloud {
  int64_t n;
  Exactly<double> xyz;
  Exactly<uint32_t> attr;
  explicit Cloud(int64_t n_) : n(n_), xyz(3 * n_), attr(n_) {}
};

// n points in a box of `half` metres: every fifth one an exact duplicate of an earlier point, every seventh one on a cell face
static void fill(Cloud& c, double voxel, double half, uint32_t seed) {
  for (int64_t i = 0; i < c.n; ++i) {
    double* q = c.xyz.p + 3 * i;
    for (int k = 0; k < 3; ++k) q[k] = (2.0 * unit(seed) - 1.0) * half;
    if (i % 7 == 3) q[i % 3] = voxel * (double)((int)(lcg(seed) % 17u) - 8);
    if (i % 5 == 4) std::memcpy(q, c.xyz.p + 3 * (lcg(seed) % (uint32_t)i), sizeof(double) * 3);
    c.attr.p[i] = lcg(seed);
  }
}

static int failed(const char* what, int set) {
  std::fprintf(stderr, "set %d: %s\n", set, what);
  return 1;
}

struct Both {
  HostMapStore store;
  VoxelMap map;
  bool with_attr, with_ev, with_mom;
  explicit Both(const MapSpec& s)
      : store(s), map(s.voxel, s.first_rows, s.max_rows, s.with_attr, s.with_ev, s.ev[0], s.ev[1], s.ev[2], s.mom), with_attr(s.with_attr),
        with_ev(s.with_ev), with_mom(s.mom > 0) {}

  bool size_agrees() {
    int64_t rows = -7;
    return store.size(&rows) == kMapOk && rows == map.size();
  }
  bool insert(const Cloud& c, bool attr, const double* R, const double* t, int* out_rc = nullptr) {
    int64_t a[2] = {-7, -7}, b[2] = {-7, -7};
    const uint32_t* w = attr ? c.attr.p : nullptr;
    const int ra = store.insert(ScanRef::host(c.xyz.p, w, c.n), R, t, &a[0], &a[1]);
    const int rb = map.insert(c.n ? c.xyz.p : nullptr, c.n, R, t, &b[0], &b[1], w);
    if (out_rc) *out_rc = ra;
    return ra == rb && std::memcmp(a, b, sizeof(a)) == 0 && size_agrees();
  }
  bool prune(const double* center, double radius, int64_t watermark, int* out_rc, int64_t* out_mark) {
    int64_t a[3] = {-7, -7, -7}, b[3] = {-7, -7, -7};
    const int ra = store.prune(center, radius, watermark, &a[0], &a[1], &a[2]);
    const int rb = map.prune(center, radius, watermark, &b[0], &b[1], &b[2]);
    *out_rc = ra;
    *out_mark = a[2];
    return ra == rb && std::memcmp(a, b, sizeof(a)) == 0 && size_agrees();
  }
  bool clearRays(const Cloud& c, const double* R, const double* t, const double* origin, double margin, int64_t watermark, int* out_rc,
                 int64_t* out_mark) {
    int64_t a[3] = {-7, -7, -7}, b[3] = {-7, -7, -7};
    const int ra = store.clearRays(ScanRef::host(c.xyz.p, nullptr, c.n), R, t, origin, margin, watermark, &a[0], &a[1], &a[2]);
    const int rb = map.clearRays(c.n ? c.xyz.p : nullptr, c.n, R, t, origin, margin, watermark, &b[0], &b[1], &b[2]);
    *out_rc = ra;
    *out_mark = a[2];
    return ra == rb && std::memcmp(a, b, sizeof(a)) == 0 && size_agrees();
  }
  // every per-point output, the columns the map lacks included (both sides must refuse them alike)
  bool query(const Cloud& c, const double* R, const double* t, int reach, double max_dist, bool ask_attr, bool ask_ev, int* out_rc) {
    Exactly<int32_t> row_a(c.n), row_b(c.n);
    Exactly<double> d2_a(c.n), d2_b(c.n);
    Exactly<uint64_t> key_a(c.n), key_b(c.n), counts_a(3), counts_b(3);
    Exactly<uint32_t> attr_a(c.n), attr_b(c.n), ev_a(c.n), ev_b(c.n);
    const int ra = store.query(ScanRef::host(c.xyz.p, nullptr, c.n), R, t, reach, max_dist, row_a.p, d2_a.p, key_a.p, ask_attr ? attr_a.p : nullptr,
                               ask_ev ? ev_a.p : nullptr, c.n, counts_a.p);
    const int rb = map.query(c.n ? c.xyz.p : nullptr, c.n, R, t, reach, max_dist, row_b.p, d2_b.p, key_b.p, ask_attr ? attr_b.p : nullptr,
                             ask_ev ? ev_b.p : nullptr, c.n, counts_b.p);
    *out_rc = ra;
    return ra == rb && row_a.same(row_b) && d2_a.same(d2_b) && key_a.same(key_b) && attr_a.same(attr_b) && ev_a.same(ev_b) &&
           counts_a.same(counts_b);
  }
  // one column of the window [first_row, size()) into exactly `capacity` rows: the store's struct against the map's own download
  bool window(int64_t first_row, int64_t capacity, int* out_rc_xyz) {
    bool ok = true;
    int64_t na, nb;
    {
      Exactly<float> a(3 * capacity), b(3 * capacity);
      MapColumns cols;
      cols.xyz = a.p;
      na = nb = -7;
      const int ra = store.download(first_row, cols, capacity, &na), rb = map.download(first_row, b.p, capacity, &nb);
      *out_rc_xyz = ra;
      ok = ok && ra == rb && na == nb && a.same(b);
    }
    {
      Exactly<uint64_t> a(capacity), b(capacity);
      MapColumns cols;
      cols.keys = a.p;
      na = nb = -7;
      ok = ok && store.download(first_row, cols, capacity, &na) == map.download_keys(first_row, b.p, capacity, &nb) && na == nb && a.same(b);
    }
    {
      Exactly<uint32_t> a(capacity), b(capacity);
      MapColumns cols;
      cols.attr = a.p;
      na = nb = -7;
      const int ra = store.download(first_row, cols, capacity, &na);
      ok = ok && ra == map.download_attr(first_row, b.p, capacity, &nb) && na == nb && a.same(b) && (with_attr || ra == kMapInvalid);
    }
    {
      Exactly<uint32_t> a(capacity), b(capacity);
      MapColumns cols;
      cols.ev = a.p;
      na = nb = -7;
      const int ra = store.download(first_row, cols, capacity, &na);
      ok = ok && ra == map.download_evidence(first_row, b.p, capacity, &nb) && na == nb && a.same(b) && (with_ev || ra == kMapInvalid);
    }
    {
      Exactly<uint64_t> a(10 * capacity), b(10 * capacity);
      MapColumns cols;
      cols.moments = a.p;
      na = nb = -7;
      const int ra = store.download(first_row, cols, capacity, &na);
      ok = ok && ra == map.download_moments(first_row, b.p, capacity, &nb) && na == nb && a.same(b) && (with_mom || ra == kMapInvalid);
    }
    for (int with_words = 0; with_words < 2; ++with_words) {  // xyz with keys, and with the words too: the rows download
      Exactly<float> xa(3 * capacity), xb(3 * capacity);
      Exactly<uint64_t> ka(capacity), kb(capacity);
      Exactly<uint32_t> wa(capacity), wb(capacity);
      MapColumns cols;
      cols.xyz = xa.p;
      cols.keys = ka.p;
      cols.attr = with_words ? wa.p : nullptr;
      na = nb = -7;
      ok = ok && store.download(first_row, cols, capacity, &na) == map.download_rows(first_row, xb.p, kb.p, with_words ? wb.p : nullptr, capacity, &nb) &&
           na == nb && xa.same(xb) && ka.same(kb) && wa.same(wb);
    }
    {
      Exactly<float> ca(3 * capacity), cb(3 * capacity), na_(3 * capacity), nb_(3 * capacity), ea(3 * capacity), eb(3 * capacity);
      Exactly<uint32_t> ka(capacity), kb(capacity);
      na = nb = -7;
      ok = ok && store.downloadSurfels(first_row, ca.p, na_.p, ea.p, ka.p, capacity, &na) ==
                     map.download_surfels(first_row, cb.p, nb_.p, eb.p, kb.p, capacity, &nb) &&
           na == nb && ca.same(cb) && na_.same(nb_) && ea.same(eb) && ka.same(kb);
    }
    return ok;
  }
  bool windows() {  // at first_row 0, in the middle and at size(); then one row short; then a struct that names no download
    const int64_t m = map.size();
    int rc = -7;
    for (const int64_t first : {int64_t(0), m / 2, m})
      if (!window(first, m - first, &rc) || rc != kMapOk) return false;
    if (m > 0 && (!window(0, m - 1, &rc) || rc != kMapCapacity)) return false;
    if (!window(m + 1, 0, &rc) || rc != kMapInvalid) return false;
    Exactly<float> x(3 * m);
    Exactly<uint32_t> e(m);
    MapColumns none, two;
    two.xyz = x.p;
    two.ev = e.p;
    int64_t n = -7;
    return store.download(0, none, m, &n) == kMapInvalid && store.download(0, two, m, &n) == kMapInvalid && n == -7;
  }
  bool confirmed(uint32_t min_e, int64_t capacity) {
    Exactly<float> xa(3 * capacity), xb(3 * capacity);
    Exactly<uint64_t> ka(capacity), kb(capacity);
    Exactly<uint32_t> wa(capacity), wb(capacity), ea(capacity), eb(capacity);
    int64_t na = -7, nb = -7;
    const int ra = store.downloadMinEvidence(min_e, xa.p, ka.p, with_attr ? wa.p : nullptr, ea.p, capacity, &na);
    const int rb = map.download_min_evidence(min_e, xb.p, kb.p, with_attr ? wb.p : nullptr, eb.p, capacity, &nb);
    return ra == rb && na == nb && xa.same(xb) && ka.same(kb) && wa.same(wb) && ea.same(eb) && (with_ev || ra == kMapInvalid);
  }
  bool take(int64_t capacity, int* out_rc) {
    int64_t ca = -7, cb = map.removed_count();
    if (store.removedCount(&ca) != kMapOk || ca != cb) return false;
    Exactly<uint64_t> ka(capacity), kb(capacity);
    Exactly<float> xa(3 * capacity), xb(3 * capacity);
    Exactly<uint32_t> wa(capacity), wb(capacity);
    int64_t na = -7, nb = -7;
    const int ra = store.takeRemoved(ka.p, xa.p, with_attr ? wa.p : nullptr, capacity, &na);
    const int rb = map.take_removed(kb.p, xb.p, with_attr ? wb.p : nullptr, capacity, &nb);
    *out_rc = ra;
    return ra == rb && na == nb && ka.same(kb) && xa.same(xb) && wa.same(wb);
  }
};

static int run(int set) {
  MapSpec spec;
  spec.voxel = 0.5;
  spec.first_rows = 64;
  spec.max_rows = 640;  // small enough for the removal log to fill below
  spec.with_attr = (set & 1) != 0;
  spec.with_ev = (set & 2) != 0;
  if (spec.with_ev) spec.ev[0] = 2, spec.ev[1] = 1, spec.ev[2] = 3;
  spec.mom = (set & 4) ? 3u : 0u;
  Both both(spec);
  if (both.store.onDevice()) return failed("a host store that says it is on the device", set);
  if (both.store.trackRemoved(true) != kMapOk) return failed("trackRemoved", set);
  both.map.track_removed(true);

  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const double Rz[9] = {0.8, -0.6, 0, 0.6, 0.8, 0, 0, 0, 1};  // (exact in binary: a rotation to the last bit)
  const double t0[3] = {0, 0, 0}, t1[3] = {0.75, -0.25, 0.125}, origin[3] = {0, 0, 0.5};
  Cloud a(320), b(270), none(0), rays(200);
  fill(a, spec.voxel, 4.0, 1u + (uint32_t)set);
  fill(b, spec.voxel, 4.0, 101u + (uint32_t)set);
  fill(rays, spec.voxel, 6.0, 201u + (uint32_t)set);
  int rc = -7;
  int64_t mark = -7;

  // three folds: a cloud with its words, an empty one, a second cloud without words at another pose
  if (!both.insert(a, true, I, t0, &rc) || rc != kMapOk) return failed("fold a", set);
  if (!both.insert(none, false, I, t0, &rc) || rc != kMapOk) return failed("fold of no point", set);
  if (!both.insert(b, false, Rz, t1, &rc) || rc != kMapOk) return failed("fold b", set);
  if (both.map.size() < 300) return failed("the folds made fewer than 300 rows", set);
  if (!both.windows()) return failed("windows after the folds", set);
  for (int reach = 0; reach < 2; ++reach) {
    if (!both.query(rays, Rz, t1, reach, 0.25, spec.with_attr, spec.with_ev, &rc) || rc != kMapOk) return failed("query", set);
    if (!both.query(none, I, t0, reach, 0.25, false, false, &rc) || rc != kMapOk) return failed("query of no point", set);
  }
  if (!both.query(rays, I, t0, 1, 0.25, !spec.with_attr, !spec.with_ev, &rc) || rc != (spec.with_attr && spec.with_ev ? kMapOk : kMapInvalid))
    return failed("query of a missing column", set);
  if (!both.query(rays, I, t0, 2, 0.25, false, false, &rc) || rc != kMapInvalid) return failed("query at reach 2", set);
  if (!both.confirmed(0, both.map.size()) || !both.confirmed(3, both.map.size())) return failed("downloadMinEvidence", set);

  // a clearing and a prune, each with a watermark inside the map; the prune takes the clearing's
  const int64_t before = both.map.size();
  if (!both.clearRays(rays, I, t0, origin, 0.0, before / 2, &rc, &mark) || rc != kMapOk) return failed("clearing", set);
  if (both.map.size() >= before && !spec.with_ev) return failed("the clearing removed nothing", set);
  if (mark <= 0) return failed("the clearing's watermark", set);
  const double center[3] = {0.5, 0.5, 0.0};
  if (!both.prune(center, 3.5, mark, &rc, &mark) || rc != kMapOk || mark <= 0) return failed("prune", set);
  if (both.map.removed_count() <= 0) return failed("nothing was logged", set);
  if (!both.windows()) return failed("windows after the removals", set);
  if (!both.clearRays(none, I, t0, origin, 0.0, mark, &rc, &mark) || rc != kMapOk) return failed("clearing of no ray", set);
  if (!both.prune(center, -1.0, 0, &rc, &mark) || rc != kMapInvalid) return failed("prune of a negative radius", set);

  // everything leaves, the cloud is folded again, until the log holds max_rows entries: the next removal is refused
  bool full = false;
  for (int round = 0; round < 8 && !full; ++round) {
    if (!both.prune(center, 1e-3, both.map.size(), &rc, &mark)) return failed("prune of everything", set);
    full = rc == kMapCapacity;
    if (!full && rc != kMapOk) return failed("prune of everything: its code", set);
    if (!full && (!both.insert(a, true, Rz, t0, &rc) || rc != kMapOk)) return failed("fold again", set);
  }
  if (!full || both.map.removed_count() < spec.max_rows) return failed("the log never filled", set);
  if (!both.clearRays(rays, I, t0, origin, 0.0, 0, &rc, &mark) || rc != kMapCapacity) return failed("clearing on a full log", set);
  rc = kMapOk;
  for (int round = 0; round < 4 && rc != kMapCapacity; ++round)  // folds go on while there is room: rows + n <= max_rows
    if (!both.insert(round % 2 ? a : b, true, I, t1, &rc) || (rc != kMapOk && rc != kMapCapacity)) return failed("a fold on a full log", set);
  if (rc != kMapCapacity) return failed("no fold was refused for max_rows", set);

  // the log: one entry short, then exactly
  const int64_t logged = both.map.removed_count();
  if (!both.take(logged - 1, &rc) || rc != kMapCapacity) return failed("take into a short buffer", set);
  if (!both.take(logged, &rc) || rc != kMapOk || both.map.removed_count() != 0) return failed("take", set);
  if (!both.prune(center, 2.0, both.map.size() / 2, &rc, &mark) || rc != kMapOk) return failed("prune after the take", set);
  if (!both.windows()) return failed("windows at the end", set);

  if (both.store.clear() != kMapOk) return failed("clear", set);
  both.map.clear();
  if (!both.size_agrees() || both.map.size() != 0 || !both.windows()) return failed("after clear", set);
  if (!both.take(0, &rc) || rc != kMapOk) return failed("take after clear", set);
  if (both.store.trackRemoved(false) != kMapOk) return failed("trackRemoved off", set);
  both.map.track_removed(false);
  if (!both.insert(b, true, Rz, t1, &rc) || rc != kMapOk || !both.windows()) return failed("a fold after clear", set);
  return 0;
}

int main() {
  for (int set = 0; set < 8; ++set)
    if (run(set)) return 1;
  std::printf("8 sets equal\n");
  return 0;
}
