// Stand-alone check of the host multi-source ingest (madicp_host_ingest_sources: csrc/host/ingest_records.cpp + ingest_records.h)
// under AddressSanitizer and UndefinedBehaviorSanitizer: compiled and run by tests/test_ingest_sources_sanitized.py.  Sets of 1 ..
// 8 sources over the layouts of tests/ingest_sources_ref.py, every source in a heap buffer of EXACTLY n * step bytes and the
// outputs in buffers of exactly the size the interface asks for: a read one byte past any source's last record, or a typed load
// from an unaligned field, ends the program with the sanitizer's report.  The results are held to the obvious field-by-field
// reading too: the order of the sources, the counts per source, the common clock's range and stamps, the extrinsic.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "madicp_host.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int fail(const char* what, int set, int s, long long i) {
  std::fprintf(stderr, "set %d source %d record %lld: %s\n", set, s, i, what);
  return 1;
}

int main() {
  const madicp_record_layout timed[] = {{16, 0, 4, 8, 12, 7},  {22, 0, 4, 8, 18, 6},   {26, 0, 4, 8, 17, 8},    {48, 0, 4, 8, 21, 6},
                                        {65, 1, 5, 9, 33, 7},  {129, 3, 7, 11, 57, 8}, {200, 0, 4, 8, 101, 6},  {256, 0, 4, 8, 247, 8}};
  const madicp_record_layout untimed[] = {{13, 1, 5, 9, 0, 0}, {12, 0, 4, 8, 0, 0}, {255, 0, 4, 8, 0, 0}};
  const int64_t counts[] = {1, 255, 257, 3, 64, 129, 2, 65};
  int sets = 0;
  for (int with_time = 0; with_time < 2; ++with_time)
    for (int n_sources = 1; n_sources <= (with_time ? 8 : 3); ++n_sources)
      for (int rot = 0; rot < 2; ++rot) {
        std::vector<madicp_record_source> src(static_cast<size_t>(n_sources));
        std::vector<unsigned char*> bufs;
        // what is expected: per record of every source, kept or not, the base-frame point and the common-clock time
        std::vector<double> want_xyz, want_tc, all_tc;
        std::vector<int64_t> want_per(static_cast<size_t>(n_sources), 0);
        int64_t total = 0;
        for (int s = 0; s < n_sources; ++s) {
          const madicp_record_layout L = with_time ? timed[(s + rot) % 8] : untimed[(s + rot) % 3];
          const int64_t n = counts[(s + 3 * rot) % 8];
          const size_t bytes = static_cast<size_t>(n) * static_cast<size_t>(L.point_step);
          unsigned char* buf = static_cast<unsigned char*>(std::malloc(bytes));  // exactly n * step
          bufs.push_back(buf);
          uint32_t seed = 991u + static_cast<uint32_t>(L.point_step) * 7u + static_cast<uint32_t>(n) + 131u * static_cast<uint32_t>(s);
          for (size_t i = 0; i < bytes; ++i) buf[i] = static_cast<unsigned char>(lcg(seed) >> 24);
          madicp_record_source& S = src[static_cast<size_t>(s)];
          std::memset(&S, 0, sizeof(S));
          S.data = buf;
          S.n_records = n;
          S.layout = L;
          // identity for even sources; for odd ones a quarter turn about z and a translation: every product is exact
          const bool identity = s % 2 == 0;
          const double R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0.5, -0.25, 1.0};
          std::memcpy(S.R, identity ? I : R, sizeof(S.R));
          if (!identity) std::memcpy(S.t, t, sizeof(S.t));
          S.min_range = 0.7 + s;
          S.max_range = 120.0;
          S.t_scale = L.t_type == 6 ? 0.5 : 1.0;  // (a power of two: the expected value below is exact whatever the order)
          S.t_offset = L.t_type == 6 ? 4.0 * s : (s == 0 ? 0.0 : 0.25 * s);
          S.kitti_correction = 0;
          for (int64_t i = 0; i < n; ++i) {
            const float r = (i % 3 == 2) ? 300.0f : 9.0f + static_cast<float>(i % 50);  // every third record beyond max_range
            const float v[3] = {r, 0.25f * static_cast<float>(i % 7), -1.0f};
            const int32_t off[3] = {L.off_x, L.off_y, L.off_z};
            for (int k = 0; k < 3; ++k) std::memcpy(buf + i * L.point_step + off[k], &v[k], 4);
            double tc = 0.0;
            if (L.t_type == 6) {
              const uint32_t tt = static_cast<uint32_t>(1000 * (n - i));
              std::memcpy(buf + i * L.point_step + L.off_t, &tt, 4);
              tc = static_cast<double>(tt) * S.t_scale + S.t_offset;
            } else if (L.t_type == 7) {
              const float tt = 0.5f * static_cast<float>(i);
              std::memcpy(buf + i * L.point_step + L.off_t, &tt, 4);
              tc = static_cast<double>(tt) * S.t_scale + S.t_offset;
            } else if (L.t_type == 8) {
              const double tt = 1024.0 + 0.125 * static_cast<double>(i);
              std::memcpy(buf + i * L.point_step + L.off_t, &tt, 8);
              tc = tt * S.t_scale + S.t_offset;
            }
            if (with_time) all_tc.push_back(tc);
            if (i % 3 == 2) continue;
            const double x = v[0], y = v[1], z = v[2];
            if (identity) {
              want_xyz.insert(want_xyz.end(), {x, y, z});
            } else {
              want_xyz.insert(want_xyz.end(), {t[0] - y, t[1] + x, t[2] + z});
            }
            want_tc.push_back(tc);
            ++want_per[static_cast<size_t>(s)];
          }
          total += n;
        }
        double t0 = HUGE_VAL, t1 = -HUGE_VAL;
        for (double tc : all_tc) {
          if (tc < t0) t0 = tc;
          if (tc > t1) t1 = tc;
        }
        double* xyz = static_cast<double*>(std::malloc(sizeof(double) * 3 * static_cast<size_t>(total)));
        double* st = static_cast<double*>(std::malloc(sizeof(double) * static_cast<size_t>(total)));
        int64_t* per = static_cast<int64_t*>(std::malloc(sizeof(int64_t) * static_cast<size_t>(n_sources)));
        int64_t kept = -1;
        double range[2] = {0, 0};
        const int rc = madicp_host_ingest_sources(src.data(), n_sources, nullptr, xyz, st, &kept, per, range);
        if (rc != 0 || kept != static_cast<int64_t>(want_tc.size())) return fail("return code or survivor count", sets, -1, kept);
        for (int s = 0; s < n_sources; ++s)
          if (per[s] != want_per[static_cast<size_t>(s)]) return fail("survivors per source", sets, s, per[s]);
        if (range[0] != t0 || range[1] != t1) return fail("range", sets, -1, 0);
        for (int64_t d = 0; d < kept; ++d) {
          for (int k = 0; k < 3; ++k)
            if (xyz[3 * d + k] != want_xyz[static_cast<size_t>(3 * d + k)]) return fail("point", sets, -1, d);
          if (with_time) {
            const double want = (t1 - t0 > 0.0) ? (want_tc[static_cast<size_t>(d)] - t0) / (t1 - t0) : NAN;
            const bool same = (want != want) ? (st[d] != st[d]) : (st[d] == want);
            if (!same) return fail("stamp", sets, -1, d);
          }
        }
        // the refusals leave the exact-size outputs alone (a write would be a sanitizer report or a changed count)
        int64_t kept2 = -7;
        madicp_record_source bad = src[0];
        bad.t_scale = 0.0;
        if (madicp_host_ingest_sources(&bad, 1, nullptr, xyz, st, &kept2, per, range) != -1 || kept2 != -7) return fail("refusal", sets, 0, 0);
        if (madicp_host_ingest_sources(src.data(), 0, nullptr, xyz, st, &kept2, per, range) != -1 || kept2 != -7) return fail("refusal", sets, 0, 1);
        std::free(per);
        std::free(st);
        std::free(xyz);
        for (unsigned char* b : bufs) std::free(b);
        ++sets;
      }
  std::printf("ingest_sources_check: %d sets clean\n", sets);
  return 0;
}
