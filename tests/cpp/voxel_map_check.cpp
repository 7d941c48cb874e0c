// Stand-alone check of the host voxel map (madicp_host_map_*: csrc/host/voxel_map.cpp + voxel_map.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer: compiled and run by tests/test_voxel_map_sanitized.py.  Every cloud lives in a heap buffer of EXACTLY
// n rows and every download goes into a buffer of EXACTLY the rows asked for (the count asked for first with a capacity of zero):
// a read past the cloud or a write past the last row ends the program with the sanitizer's report.  The results are held to the
// obvious reading of the rule too: a brute-force list of the cells seen so far over the same positions, across the frames.
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
  std::fprintf(stderr, "set %d frame/row %lld: %s\n", set, i, what);
  return 1;
}

int main() {
  const int64_t sizes[] = {1, 2, 63, 64, 65, 255, 257, 1024, 1025, 3000};
  const double voxels[] = {1e-3, 0.5, 50.0};
  // a quarter turn about z and a translation (every product exact), and the identity
  const double Rq[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tq[3] = {0.5, -0.25, 1.0}, t0[3] = {0, 0, 0};
  int sets = 0;
  for (int64_t n : sizes)
    for (double voxel : voxels)
      for (int kind = 0; kind < 3; ++kind) {
        // initial_rows 1: every growth of the twin's storage happens; max_rows: the four frames always fit
        madicp_host_map* map = nullptr;
        if (madicp_host_map_create(voxel, 1, 4 * n, &map) != MADICP_OK || !map) return fail("create", sets, 0);
        std::vector<float> want;
        std::vector<int64_t> cx, cy, cz;
        uint32_t seed = 977u + 31u * static_cast<uint32_t>(n) + static_cast<uint32_t>(sets);
        for (int frame = 0; frame < 4; ++frame) {
          const bool turn = ((sets + frame) % 2) == 1;
          const double* R = turn ? Rq : I;
          const double* t = turn ? tq : t0;
          double* xyz = static_cast<double*>(std::malloc(sizeof(double) * 3 * static_cast<size_t>(n)));  // exactly n rows
          for (int64_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) {
              double v;
              if (kind == 0) v = (unit(seed) - 0.5) * 40.0;                                    // spread out
              else if (kind == 1) v = 0.5 * static_cast<double>((int)(lcg(seed) >> 28) - 8);  // on cell faces, many duplicates
              else v = 1e-5 + 8e-4 * unit(seed);                                              // one cell
              xyz[3 * i + k] = v;
            }
          if (kind == 0 && n > 2) {  // rows that are no candidates
            xyz[3 * (n / 2)] = NAN;
            xyz[3 * (n - 1) + 1] = HUGE_VAL;
          }
          const int64_t before = static_cast<int64_t>(want.size() / 3);
          for (int64_t i = 0; i < n; ++i) {
            const double* p = xyz + 3 * i;
            double q[3], f[3];
            bool keep = true;
            for (int r = 0; r < 3; ++r) {
              q[r] = t[r] + (R[3 * r] * p[0] + (R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]));
              f[r] = std::floor(q[r] / voxel);
              if (!(f[r] >= -1048576.0 && f[r] < 1048576.0)) keep = false;
            }
            if (!keep) continue;
            const int64_t a = static_cast<int64_t>(f[0]), b = static_cast<int64_t>(f[1]), c = static_cast<int64_t>(f[2]);
            for (size_t k = 0; k < cx.size() && keep; ++k)
              if (cx[k] == a && cy[k] == b && cz[k] == c) keep = false;
            if (!keep) continue;
            cx.push_back(a);
            cy.push_back(b);
            cz.push_back(c);
            for (int r = 0; r < 3; ++r) want.push_back(static_cast<float>(q[r]));
          }
          const int64_t m_want = static_cast<int64_t>(want.size() / 3);
          int64_t added = -7, rows = -7;
          // refusals first: they leave everything alone
          double Rbad[9];
          std::memcpy(Rbad, R, sizeof(Rbad));
          Rbad[4] = NAN;
          if (madicp_host_map_insert(map, xyz, n, Rbad, t, &added, &rows) != MADICP_ERR_INVALID) return fail("refusal", sets, 0);
          if (madicp_host_map_insert(map, nullptr, n, R, t, &added, &rows) != MADICP_ERR_INVALID) return fail("refusal", sets, 1);
          if (madicp_host_map_insert(map, xyz, n, R, t, nullptr, &rows) != MADICP_ERR_INVALID) return fail("refusal", sets, 2);
          if (added != -7 || rows != -7) return fail("refusal wrote", sets, 3);
          int rc = madicp_host_map_insert(map, xyz, n, R, t, &added, &rows);
          if (rc != MADICP_OK || added != m_want - before || rows != m_want) return fail("insert", sets, frame);
          std::free(xyz);
          // what this frame added: the count with a capacity of zero, then a buffer of exactly those rows
          float* none = static_cast<float*>(std::malloc(sizeof(float)));
          none[0] = -77.5f;
          int64_t m = -7;
          rc = madicp_host_map_download_f32(map, before, none, 0, &m);
          if (m != added || rc != (added > 0 ? MADICP_ERR_CAPACITY : MADICP_OK) || none[0] != -77.5f) return fail("capacity refusal", sets, frame);
          if (madicp_host_map_download_f32(map, m_want + 1, none, 0, &m) != MADICP_ERR_INVALID) return fail("first_row refusal", sets, frame);
          float* out = static_cast<float*>(std::malloc(sizeof(float) * 3 * static_cast<size_t>(added > 0 ? added : 1)));
          rc = madicp_host_map_download_f32(map, before, out, added, &m);
          if (rc != MADICP_OK || m != added) return fail("download", sets, frame);
          if (added > 0 && std::memcmp(out, want.data() + 3 * before, sizeof(float) * 3 * static_cast<size_t>(added)) != 0)
            return fail("window rows", sets, frame);
          std::free(out);
          std::free(none);
        }
        // the whole map, exactly its rows; then a cloud one point too large is refused for capacity with the map unchanged
        const int64_t m_all = static_cast<int64_t>(want.size() / 3);
        int64_t m = -7;
        if (madicp_host_map_size(map, &m) != MADICP_OK || m != m_all) return fail("size", sets, m);
        float* all = static_cast<float*>(std::malloc(sizeof(float) * 3 * static_cast<size_t>(m_all > 0 ? m_all : 1)));
        if (madicp_host_map_download_f32(map, 0, all, m_all, &m) != MADICP_OK || m != m_all) return fail("download all", sets, m);
        if (m_all > 0 && std::memcmp(all, want.data(), sizeof(float) * 3 * static_cast<size_t>(m_all)) != 0) return fail("rows", sets, -1);
        std::free(all);
        {
          const int64_t over = 4 * n - m_all + 1;  // one point more than max_rows leaves room for
          double* xyz = static_cast<double*>(std::calloc(3 * static_cast<size_t>(over), sizeof(double)));
          int64_t added = -7, rows = -7;
          if (madicp_host_map_insert(map, xyz, over, I, t0, &added, &rows) != MADICP_ERR_CAPACITY || added != -7 || rows != -7)
            return fail("max_rows refusal", sets, 0);
          if (madicp_host_map_size(map, &m) != MADICP_OK || m != m_all) return fail("max_rows refusal changed the map", sets, m);
          std::free(xyz);
        }
        if (madicp_host_map_clear(map) != MADICP_OK || madicp_host_map_size(map, &m) != MADICP_OK || m != 0) return fail("clear", sets, m);
        madicp_host_map_destroy(map);
        ++sets;
      }
  std::printf("voxel_map_check: %d sets clean\n", sets);
  return 0;
}
