// Stand-alone check of the host export (madicp_host_cloud_export_f32: csrc/host/cloud_export.cpp + cloud_export.h) under
// AddressSanitizer and UndefinedBehaviorSanitizer: compiled and run by tests/test_cloud_export_sanitized.py.  Every input lives
// in a heap buffer of EXACTLY n rows and every output in a buffer of EXACTLY the M rows the call needs (asked for first with a
// capacity of zero): a read past the cloud or a write past row M ends the program with the sanitizer's report.  The results are
// held to the obvious reading of the rule too: a brute-force "first index of every cell" over the same positions.
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
  std::fprintf(stderr, "set %d row %lld: %s\n", set, i, what);
  return 1;
}

int main() {
  const int64_t sizes[] = {1, 2, 63, 64, 65, 255, 257, 1024, 1025, 3000};
  const double voxels[] = {0.0, 1e-3, 0.5, 50.0};
  // a quarter turn about z and a translation (every product exact), and the identity
  const double Rq[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tq[3] = {0.5, -0.25, 1.0}, t0[3] = {0, 0, 0};
  int sets = 0;
  for (int64_t n : sizes)
    for (double voxel : voxels)
      for (int kind = 0; kind < 3; ++kind) {
        const bool turn = (sets % 2) == 1;
        const double* R = turn ? Rq : I;
        const double* t = turn ? tq : t0;
        double* xyz = static_cast<double*>(std::malloc(sizeof(double) * 3 * static_cast<size_t>(n)));  // exactly n rows
        uint32_t seed = 4242u + 17u * static_cast<uint32_t>(n) + static_cast<uint32_t>(sets);
        for (int64_t i = 0; i < n; ++i)
          for (int k = 0; k < 3; ++k) {
            double v;
            if (kind == 0) v = (unit(seed) - 0.5) * 40.0;                       // spread out
            else if (kind == 1) v = 0.5 * static_cast<double>((int)(lcg(seed) >> 28) - 8);  // on cell faces, many duplicates
            else v = 1e-5 + 8e-4 * unit(seed);                                   // one cell
            xyz[3 * i + k] = v;
          }
        if (kind == 0 && n > 2) {  // rows that are no candidates
          xyz[3 * (n / 2)] = NAN;
          xyz[3 * (n - 1) + 1] = HUGE_VAL;
        }
        // what is expected: positions by the stated order, the first index of every cell
        std::vector<float> want;
        std::vector<int64_t> cx, cy, cz;
        for (int64_t i = 0; i < n; ++i) {
          const double* p = xyz + 3 * i;
          double q[3];
          for (int r = 0; r < 3; ++r) q[r] = t[r] + (R[3 * r] * p[0] + (R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2]));
          bool keep = true;
          if (voxel > 0.0) {
            double f[3];
            for (int r = 0; r < 3; ++r) {
              f[r] = std::floor(q[r] / voxel);
              if (!(f[r] >= -1048576.0 && f[r] < 1048576.0)) keep = false;
            }
            if (keep) {
              const int64_t a = static_cast<int64_t>(f[0]), b = static_cast<int64_t>(f[1]), c = static_cast<int64_t>(f[2]);
              for (size_t k = 0; k < cx.size() && keep; ++k)
                if (cx[k] == a && cy[k] == b && cz[k] == c) keep = false;
              if (keep) {
                cx.push_back(a);
                cy.push_back(b);
                cz.push_back(c);
              }
            }
          }
          if (keep)
            for (int r = 0; r < 3; ++r) want.push_back(static_cast<float>(q[r]));
        }
        const int64_t m_want = static_cast<int64_t>(want.size() / 3);
        // the count first: capacity 0 (a one-float buffer that must stay untouched), then a buffer of exactly M rows
        float* none = static_cast<float*>(std::malloc(sizeof(float)));
        none[0] = -77.5f;
        int64_t m = -7;
        int rc = madicp_host_cloud_export_f32(xyz, n, R, t, voxel, none, 0, &m);
        if (m != m_want) return fail("row count", sets, m);
        if (rc != (m_want > 0 ? MADICP_ERR_CAPACITY : MADICP_OK) || none[0] != -77.5f) return fail("capacity refusal", sets, rc);
        float* out = static_cast<float*>(std::malloc(sizeof(float) * 3 * static_cast<size_t>(m_want > 0 ? m_want : 1)));
        int64_t m2 = -7;
        rc = madicp_host_cloud_export_f32(xyz, n, R, t, voxel, out, m_want, &m2);
        if (rc != MADICP_OK || m2 != m_want) return fail("return code", sets, rc);
        if (m_want > 0 && std::memcmp(out, want.data(), sizeof(float) * 3 * static_cast<size_t>(m_want)) != 0) return fail("rows", sets, -1);
        // refusals leave everything alone
        int64_t m3 = -7;
        double Rbad[9];
        std::memcpy(Rbad, R, sizeof(Rbad));
        Rbad[4] = NAN;
        if (madicp_host_cloud_export_f32(xyz, n, Rbad, t, voxel, none, 0, &m3) != MADICP_ERR_INVALID || m3 != -7) return fail("refusal", sets, 0);
        if (madicp_host_cloud_export_f32(xyz, n, R, t, -1.0, none, 0, &m3) != MADICP_ERR_INVALID || m3 != -7) return fail("refusal", sets, 1);
        if (madicp_host_cloud_export_f32(nullptr, n, R, t, voxel, none, 0, &m3) != MADICP_ERR_INVALID || m3 != -7) return fail("refusal", sets, 2);
        if (none[0] != -77.5f) return fail("refusal wrote", sets, 3);
        std::free(out);
        std::free(none);
        std::free(xyz);
        ++sets;
      }
  std::printf("cloud_export_check: %d sets clean\n", sets);
  return 0;
}
