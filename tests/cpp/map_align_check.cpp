// Stand-alone check of the host voxel map's registration (madicp_host_map_register: csrc/host/voxel_map.cpp + voxel_map.h, the rule
// of csrc/common/map_align.h) under AddressSanitizer and UndefinedBehaviorSanitizer: compiled and run by
// tests/test_map_align_sanitized.py.  Every cloud lives in a heap buffer of EXACTLY n rows, the per-point outputs in buffers of
// EXACTLY n entries, trace and counts in buffers of EXACTLY iterations + 1 rows: a write past the end ends the program with the
// sanitizer's report.  The answers are held to the rule read literally: the row is madicp_host_map_query's, the terms are computed
// here from madicp_host_map_download_surfels, and the sum is the RECURSIVE form of the tree — sum(lo, size) = sum(lo, size / 2) +
// sum(lo + size / 2, size / 2) over the power of two that covers n — where the product runs it level by level.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "madicp_host.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t& s) { return (lcg(s) >> 8) / 16777216.0; }
static double gauss(uint32_t& s) { return (unit(s) + unit(s) + unit(s) + unit(s) - 2.0) * 1.7320508; }

static int fail(const char* what, int set, long long i) {
  std::fprintf(stderr, "set %d step %lld: %s\n", set, i, what);
  return 1;
}

template <class T>
static T* exactly(int64_t n) {  // (a zero-byte block is legal, and every write to it is out of bounds)
  return static_cast<T*>(std::malloc(sizeof(T) * static_cast<size_t>(n)));
}

static const double kI[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kZ[3] = {0, 0, 0};

// a room corner: point i on plane i % 3, noise along the normal
static void corner(double* p, int64_t n, uint32_t seed, double margin) {
  uint32_t s = seed;
  const double o[3] = {0.23, 0.31, 0.17};
  for (int64_t i = 0; i < n; ++i) {
    for (int a = 0; a < 3; ++a) p[3 * i + a] = o[a] + margin + unit(s) * (5.0 - 2.0 * margin);
    p[3 * i + i % 3] = o[i % 3] + 0.02 * gauss(s);
  }
}

struct Surfels {
  std::vector<float> centroid, normal, eig;
  std::vector<uint32_t> count;
};

static void terms_of(const double* p, const double* X, const Surfels& S, int32_t j, double rho, double* x, double* e_out) {
  const double* R = X;
  const double* t = X + 9;
  double q[3];
  for (int a = 0; a < 3; ++a) q[a] = t[a] + (R[3 * a] * p[0] + (R[3 * a + 1] * p[1] + R[3 * a + 2] * p[2]));
  const double n0 = S.normal[3 * j], n1 = S.normal[3 * j + 1], n2 = S.normal[3 * j + 2];
  const double e = n0 * (q[0] - S.centroid[3 * j]) + (n1 * (q[1] - S.centroid[3 * j + 1]) + n2 * (q[2] - S.centroid[3 * j + 2]));
  double J[6];
  for (int k = 0; k < 3; ++k) J[k] = n0 * R[k] + (n1 * R[3 + k] + n2 * R[6 + k]);
  J[3] = p[1] * J[2] - p[2] * J[1];
  J[4] = p[2] * J[0] - p[0] * J[2];
  J[5] = p[0] * J[1] - p[1] * J[0];
  const double a = std::fabs(e), s = a > rho ? rho / a : 1.0;
  int v = 0;
  for (int c = 0; c < 6; ++c)
    for (int r = c; r < 6; ++r) x[v++] = (s * J[r]) * J[c];
  for (int r = 0; r < 6; ++r) x[21 + r] = (s * J[r]) * e;
  x[27] = (s * e) * e;
  *e_out = e;
}

static void tree(const std::vector<double>& x, int64_t n, int64_t lo, int64_t size, double* out) {
  if (size == 1) {
    for (int c = 0; c < 28; ++c) out[c] = lo < n ? x[28 * lo + c] : 0.0;
    return;
  }
  double a[28], b[28];
  tree(x, n, lo, size / 2, a);
  if (lo + size / 2 < n)
    tree(x, n, lo + size / 2, size / 2, b);
  else
    for (int c = 0; c < 28; ++c) b[c] = 0.0;
  for (int c = 0; c < 28; ++c) out[c] = a[c] + b[c];
}

static int check_set(int set, madicp_host_map* map, const Surfels& S, int64_t n, int iterations, const madicp_map_align_params& P, bool per_point) {
  double* cloud = exactly<double>(3 * n);
  corner(cloud, n, 1000u + static_cast<uint32_t>(n), 0.5);
  const double th = 0.012;
  const double R[9] = {std::cos(th), -std::sin(th), 0, std::sin(th), std::cos(th), 0, 0, 0, 1}, t[3] = {0.03, -0.02, 0.04};
  const int64_t k1 = iterations + 1;
  double* trace = exactly<double>(40 * k1);
  uint64_t* counts = exactly<uint64_t>(4 * k1);
  int32_t* row = per_point ? exactly<int32_t>(n) : nullptr;
  double* e = per_point ? exactly<double>(n) : nullptr;
  double oR[9], ot[3];
  int rc = madicp_host_map_register(map, cloud, n, R, t, &P, iterations, oR, ot, trace, counts, row, e, n);
  int bad = 0;
  if (rc != MADICP_OK) bad = fail("register refused", set, rc);
  for (int64_t k = 0; !bad && k < k1; ++k) {
    const double* X = trace + 40 * k;
    if (k == 0 && (std::memcmp(X, R, sizeof(R)) != 0 || std::memcmp(X + 9, t, sizeof(t)) != 0)) bad = fail("trace row 0 is not the given pose", set, k);
    int32_t* qrow = exactly<int32_t>(n);
    double* qd2 = exactly<double>(n);
    uint64_t qc[3];
    if (madicp_host_map_query(map, cloud, n, X, X + 9, P.reach, P.max_dist, qrow, qd2, nullptr, nullptr, nullptr, n, qc) != MADICP_OK)
      bad = fail("query refused", set, k);
    std::vector<double> x(28 * static_cast<size_t>(n > 0 ? n : 1), 0.0);
    uint64_t inliers = 0;
    for (int64_t i = 0; !bad && i < n; ++i) {
      const int32_t j = qrow[i];
      double ei = 0.0;
      if (j >= 0 && qd2[i] <= P.max_dist * P.max_dist && S.count[j] >= P.min_count && static_cast<double>(S.eig[3 * j + 1]) > 0.0 &&
          static_cast<double>(S.eig[3 * j]) <= P.flat * static_cast<double>(S.eig[3 * j + 1])) {
        terms_of(cloud + 3 * i, X, S, j, P.rho, &x[28 * i], &ei);
        ++inliers;
      }
      if (per_point && (row[i] != j || std::memcmp(&e[i], &ei, sizeof(double)) != 0)) bad = fail("per-point row or e", set, i);
    }
    double total[28];
    int64_t size = 1;
    while (size < n) size *= 2;
    tree(x, n, 0, size, total);
    for (int c = 0; !bad && c < 28; ++c)
      if (!(total[c] == X[12 + c])) bad = fail("a sum is not the tree's", set, c);
    if (!bad && (counts[4 * k] != qc[0] || counts[4 * k + 1] != qc[1] || counts[4 * k + 2] != qc[2] || counts[4 * k + 3] != inliers))
      bad = fail("counts", set, k);
    if (!bad && k == k1 - 1 && (std::memcmp(X, oR, sizeof(oR)) != 0 || std::memcmp(X + 9, ot, sizeof(ot)) != 0))
      bad = fail("the last trace row is not at the returned pose", set, k);
    if (!bad && k == 1 && n >= 256 && !(X[39] < trace[39])) bad = fail("round 0 did not reduce chi2", set, k);
    std::free(qrow);
    std::free(qd2);
  }
  std::free(cloud);
  std::free(trace);
  std::free(counts);
  std::free(row);
  std::free(e);
  return bad;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  madicp_host_map* map = nullptr;
  if (madicp_host_map_create_mom(0.5, 64, 1 << 20, 0, nullptr, 1u << 20, &map) != MADICP_OK) return fail("create", 0, 0);
  for (uint32_t f = 0; f < 4; ++f) {
    const int64_t n = 6000;
    double* pts = exactly<double>(3 * n);
    corner(pts, n, 7u + f, 0.0);
    int64_t added = 0, rows = 0;
    if (madicp_host_map_insert(map, pts, n, kI, kZ, &added, &rows) != MADICP_OK) return fail("insert", 0, f);
    std::free(pts);
  }
  int64_t m = 0, got = 0;
  madicp_host_map_size(map, &m);
  Surfels S;
  S.centroid.resize(3 * m);
  S.normal.resize(3 * m);
  S.eig.resize(3 * m);
  S.count.resize(m);
  if (madicp_host_map_download_surfels(map, 0, S.centroid.data(), S.normal.data(), S.eig.data(), S.count.data(), m, &got) != MADICP_OK || got != m)
    return fail("surfels", 0, m);
  const madicp_map_align_params neutral{1, inf, inf, 3, 1.0}, gated{1, 0.45, 0.03, 40, 0.3}, own{0, 0.3, 0.05, 3, 0.5};
  int sets = 0;
  for (int64_t n : {0, 1, 2, 63, 64, 65, 255, 256, 257, 4097})
    for (const madicp_map_align_params* P : {&neutral, &gated, &own})
      for (int iterations : {0, 3}) {
        if (check_set(sets, map, S, n, iterations, *P, iterations == 0)) return 1;
        ++sets;
      }
  // refusals write nothing: buffers of ONE entry would be overrun by any write of a real size, and keep their pattern
  double* cloud = exactly<double>(3 * 65);
  corner(cloud, 65, 5u, 0.5);
  double oR[9], ot[3], trace[40], e1[1] = {7.0};
  uint64_t counts[4] = {7, 7, 7, 7};
  int32_t row1[1] = {7};
  for (int i = 0; i < 9; ++i) oR[i] = 7.0;
  for (int i = 0; i < 3; ++i) ot[i] = 7.0;
  for (int i = 0; i < 40; ++i) trace[i] = 7.0;
  madicp_map_align_params bad = neutral;
  bad.min_count = 2;
  if (madicp_host_map_register(map, cloud, 65, kI, kZ, &bad, 0, oR, ot, trace, counts, nullptr, nullptr, 0) != MADICP_ERR_INVALID) return fail("min_count 2", sets, 0);
  if (madicp_host_map_register(map, cloud, 65, kI, kZ, &neutral, 65, oR, ot, trace, counts, nullptr, nullptr, 0) != MADICP_ERR_INVALID) return fail("65 rounds", sets, 0);
  if (madicp_host_map_register(map, cloud, 65, kI, kZ, &neutral, 1, oR, ot, trace, counts, row1, nullptr, 65) != MADICP_ERR_INVALID) return fail("rows with rounds", sets, 0);
  if (madicp_host_map_register(map, cloud, 65, kI, kZ, &neutral, 0, oR, ot, trace, counts, row1, e1, 1) != MADICP_ERR_CAPACITY) return fail("capacity", sets, 0);
  if (oR[0] != 7.0 || ot[2] != 7.0 || trace[39] != 7.0 || counts[3] != 7 || row1[0] != 7 || e1[0] != 7.0) return fail("a refusal wrote", sets, 0);
  std::free(cloud);
  madicp_host_map_destroy(map);
  std::printf("%d sets clean\n", sets);
  return 0;
}
