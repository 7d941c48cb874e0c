// Stand-alone check of the host records ingest (madicp_host_ingest_records: csrc/host/ingest_records.cpp + ingest_records.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer: compiled and run by tests/test_ingest_records_sanitized.py.  Every layout of
// tests/ingest_records_ref.py at 1, 255 and 257 records, the input in a heap buffer of EXACTLY n * step bytes and the outputs
// in buffers of exactly the size the interface asks for: a read one byte past the records, or a typed load from an unaligned
// field, ends the program with the sanitizer's report.  The results are held to the obvious field-by-field reading too.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "madicp_host.h"

typedef madicp_record_layout RecordLayout;

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

int main() {
  const RecordLayout layouts[] = {{12, 0, 4, 8, 0, 0},    {13, 1, 5, 9, 0, 0},    {16, 0, 4, 8, 12, 7},
                                  {22, 0, 4, 8, 18, 7},   {26, 0, 4, 8, 18, 8},   {32, 8, 4, 0, 24, 8},
                                  {48, 0, 4, 8, 20, 6},   {255, 0, 4, 8, 251, 6}, {256, 0, 4, 8, 248, 8}};
  const int64_t counts[] = {1, 255, 257};
  int cases = 0;
  for (const RecordLayout& L : layouts)
    for (int64_t n : counts)
      for (int kitti = 0; kitti < 2; ++kitti) {
        const size_t bytes = static_cast<size_t>(n) * static_cast<size_t>(L.point_step);
        unsigned char* buf = static_cast<unsigned char*>(std::malloc(bytes));  // exactly n * step
        uint32_t seed = 12345u + static_cast<uint32_t>(L.point_step) * 7u + static_cast<uint32_t>(n);
        for (size_t i = 0; i < bytes; ++i) buf[i] = static_cast<unsigned char>(lcg(seed) >> 24);
        std::vector<float> xs(static_cast<size_t>(n) * 3);
        std::vector<double> ts(static_cast<size_t>(n));
        int64_t want_kept = 0;
        for (int64_t i = 0; i < n; ++i) {
          const float r = (i % 3 == 2) ? 300.0f : 5.0f + static_cast<float>(i % 50);  // every third record beyond max_range
          const float v[3] = {r, 0.25f * static_cast<float>(i % 7), -1.0f};
          const int32_t off[3] = {L.off_x, L.off_y, L.off_z};
          for (int k = 0; k < 3; ++k) {
            std::memcpy(buf + i * L.point_step + off[k], &v[k], 4);
            xs[static_cast<size_t>(3 * i + k)] = v[k];
          }
          if (i % 3 != 2) ++want_kept;
          if (L.t_type == 6) {
            const uint32_t t = static_cast<uint32_t>(1000 * (n - i));
            std::memcpy(buf + i * L.point_step + L.off_t, &t, 4);
            ts[static_cast<size_t>(i)] = static_cast<double>(t);
          } else if (L.t_type == 7) {
            const float t = 0.001f * static_cast<float>(i);
            std::memcpy(buf + i * L.point_step + L.off_t, &t, 4);
            ts[static_cast<size_t>(i)] = static_cast<double>(t);
          } else if (L.t_type == 8) {
            const double t = 1.7e9 + 1e-4 * static_cast<double>(i);
            std::memcpy(buf + i * L.point_step + L.off_t, &t, 8);
            ts[static_cast<size_t>(i)] = t;
          }
        }
        double* xyz = static_cast<double*>(std::malloc(sizeof(double) * 3 * static_cast<size_t>(n)));
        double* st = static_cast<double*>(std::malloc(sizeof(double) * static_cast<size_t>(n)));
        int64_t kept = -1;
        double range[2] = {0, 0};
        const int rc = madicp_host_ingest_records(buf, n, &L, 0.7, 120.0, kitti, nullptr, xyz, st, &kept, range);
        if (rc != 0 || kept != want_kept) {
          std::fprintf(stderr, "step %d n %lld: rc %d kept %lld, expected %lld\n", L.point_step, static_cast<long long>(n), rc,
                       static_cast<long long>(kept), static_cast<long long>(want_kept));
          return 1;
        }
        double t0 = HUGE_VAL, t1 = -HUGE_VAL;
        if (L.t_type != 0)
          for (int64_t i = 0; i < n; ++i) {
            if (ts[static_cast<size_t>(i)] < t0) t0 = ts[static_cast<size_t>(i)];
            if (ts[static_cast<size_t>(i)] > t1) t1 = ts[static_cast<size_t>(i)];
          }
        if (range[0] != t0 || range[1] != t1) {
          std::fprintf(stderr, "step %d n %lld: range %g %g, expected %g %g\n", L.point_step, static_cast<long long>(n), range[0], range[1], t0, t1);
          return 1;
        }
        int64_t d = 0;
        for (int64_t i = 0; i < n; ++i) {
          if (i % 3 == 2) continue;
          if (!kitti)
            for (int k = 0; k < 3; ++k)
              if (xyz[3 * d + k] != static_cast<double>(xs[static_cast<size_t>(3 * i + k)])) {
                std::fprintf(stderr, "step %d n %lld: point %lld differs\n", L.point_step, static_cast<long long>(n), static_cast<long long>(i));
                return 1;
              }
          if (L.t_type != 0) {
            const double want = (t1 - t0 > 0.0) ? (ts[static_cast<size_t>(i)] - t0) / (t1 - t0) : NAN;
            const bool same = (want != want) ? (st[d] != st[d]) : (st[d] == want);
            if (!same) {
              std::fprintf(stderr, "step %d n %lld: stamp %lld is %g, expected %g\n", L.point_step, static_cast<long long>(n),
                           static_cast<long long>(i), st[d], want);
              return 1;
            }
          }
          ++d;
        }
        std::free(st);
        std::free(xyz);
        std::free(buf);
        ++cases;
      }
  std::printf("ingest_records_check: %d cases clean\n", cases);
  return 0;
}
