// The host twins of the per-point attribute (madicp_host_ingest_sources_attr, madicp_host_cloud_export_f32_attr, madicp_host_map_*_attr:
// include/madicp_host.h) as a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_attribute_sanitized.py
// compiles this file with csrc/host/ingest_records.cpp, cloud_export.cpp and voxel_map.cpp and runs it).  Every buffer is a heap
// allocation of EXACTLY the bytes the interface promises to touch — records n * step, outputs one row / word per record or per row
// asked for — so a field read past the last record's last byte or a word written past the last row is reported.  The results are
// checked against a byte-wise restatement in this file.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "madicp_host.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);            \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

int width_of(int type) { return type <= 2 ? 1 : (type <= 4 ? 2 : 4); }

// n records of `step` bytes, exactly: random bytes, then x / y / z at 0 / 4 / 8 — every third record beyond the range (dropped)
std::unique_ptr<unsigned char[]> records(int64_t n, int step, uint32_t seed, std::vector<bool>* keep) {
  std::unique_ptr<unsigned char[]> buf(new unsigned char[static_cast<size_t>(n) * step]);
  for (int64_t i = 0; i < n * step; ++i) buf[i] = static_cast<unsigned char>(lcg(seed) >> 24);
  keep->assign(static_cast<size_t>(n), true);
  for (int64_t i = 0; i < n; ++i) {
    const bool k = i % 3 != 1;
    const float xyz[3] = {k ? 5.0f + static_cast<float>(i % 7) : 500.0f, static_cast<float>(i % 5) - 2.0f, 0.25f};
    std::memcpy(buf.get() + i * step, xyz, 12);
    (*keep)[static_cast<size_t>(i)] = k;
  }
  return buf;
}

uint32_t word_of(const unsigned char* p, int type) {
  uint32_t w = 0;
  for (int b = 0; b < width_of(type); ++b) w |= static_cast<uint32_t>(p[b]) << (8 * b);
  return w;
}

madicp_record_source source_of(const unsigned char* data, int64_t n, int step) {
  madicp_record_source s{};
  s.data = data;
  s.n_records = n;
  s.layout = madicp_record_layout{step, 0, 4, 8, 0, MADICP_T_NONE};
  s.R[0] = s.R[4] = s.R[8] = 1.0;
  s.min_range = 1.0;
  s.max_range = 100.0;
  s.t_scale = 1.0;
  return s;
}

int sets = 0;

// two sources of one step, the field of `type` at `off`: the survivors' words against the restatement
void ingest_set(int step, int type, int off, int64_t n0, int64_t n1) {
  std::vector<bool> k0, k1;
  auto r0 = records(n0, step, 17u * step + type, &k0), r1 = records(n1, step, 29u * step + off, &k1);
  const madicp_record_source src[2] = {source_of(r0.get(), n0, step), source_of(r1.get(), n1, step)};
  const madicp_attr_field fields[2] = {{off, type}, {off, type}};
  const int64_t total = n0 + n1;
  std::unique_ptr<double[]> xyz(new double[3 * static_cast<size_t>(total)]);
  std::unique_ptr<uint32_t[]> words(new uint32_t[static_cast<size_t>(total)]);
  int64_t kept = -1, per[2] = {-1, -1};
  CHECK(madicp_host_ingest_sources_attr(src, 2, fields, nullptr, xyz.get(), nullptr, words.get(), &kept, per, nullptr) == 0);
  int64_t at = 0;
  for (int s = 0; s < 2; ++s) {
    const unsigned char* rec = s == 0 ? r0.get() : r1.get();
    const std::vector<bool>& keep = s == 0 ? k0 : k1;
    for (size_t i = 0; i < keep.size(); ++i) {
      if (!keep[i]) continue;
      CHECK(at < kept && words[at] == word_of(rec + i * step + off, type));
      ++at;
    }
  }
  CHECK(at == kept && per[0] + per[1] == kept);
  ++sets;
}

void ingest_refusals() {
  std::vector<bool> k;
  auto r = records(10, 22, 3, &k);
  const madicp_record_source src[2] = {source_of(r.get(), 10, 22), source_of(r.get(), 10, 22)};
  std::unique_ptr<double[]> xyz(new double[60]);
  std::unique_ptr<uint32_t[]> words(new uint32_t[20]);
  for (int i = 0; i < 20; ++i) words[i] = 0xdeadbeefu;
  int64_t kept = -5;
  const madicp_attr_field bad[][2] = {{{19, 7}, {3, 7}}, {{3, 7}, {3, 6}}, {{3, 7}, {0, 0}}, {{0, 0}, {3, 7}}, {{3, 8}, {3, 8}}, {{-1, 2}, {0, 2}},
                                      {{21, 4}, {0, 4}}, {{22, 1}, {0, 1}}};
  for (const auto& f : bad) CHECK(madicp_host_ingest_sources_attr(src, 2, f, nullptr, xyz.get(), nullptr, words.get(), &kept, nullptr, nullptr) == -1);
  const madicp_attr_field good[2] = {{18, 7}, {18, 7}};
  CHECK(madicp_host_ingest_sources_attr(src, 2, good, nullptr, xyz.get(), nullptr, nullptr, &kept, nullptr, nullptr) == -1);
  CHECK(kept == -5);
  for (int i = 0; i < 20; ++i) CHECK(words[i] == 0xdeadbeefu);
  CHECK(madicp_host_ingest_sources_attr(src, 2, good, nullptr, xyz.get(), nullptr, words.get(), &kept, nullptr, nullptr) == 0 && kept == 14);
  CHECK(madicp_host_ingest_sources_attr(src, 2, nullptr, nullptr, xyz.get(), nullptr, nullptr, &kept, nullptr, nullptr) == 0 && kept == 14);
  ++sets;
}

// n points on a line, two per 1 m cell: export and map keep the FIRST point of every cell and its word
void export_and_map_set(int64_t n) {
  const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  std::unique_ptr<double[]> xyz(new double[3 * static_cast<size_t>(n)]);
  std::unique_ptr<uint32_t[]> attr(new uint32_t[static_cast<size_t>(n)]);
  for (int64_t i = 0; i < n; ++i) {
    xyz[3 * i] = 0.25 + 0.5 * static_cast<double>(i);
    xyz[3 * i + 1] = xyz[3 * i + 2] = 0.25;
    attr[i] = 1000u + static_cast<uint32_t>(i);
  }
  const int64_t cells = (n + 1) / 2;
  {  // voxel 0: every point; exact capacity
    std::unique_ptr<float[]> rows(new float[3 * static_cast<size_t>(n)]);
    std::unique_ptr<uint32_t[]> w(new uint32_t[static_cast<size_t>(n)]);
    int64_t m = -1;
    CHECK(madicp_host_cloud_export_f32_attr(xyz.get(), attr.get(), n, R, t, 0.0, rows.get(), w.get(), n, &m) == MADICP_OK && m == n);
    for (int64_t i = 0; i < n; ++i) CHECK(w[i] == attr[i]);
  }
  {  // voxel 1: buffers of exactly the rows that go out; one row fewer is refused and writes nothing
    std::unique_ptr<float[]> rows(new float[3 * static_cast<size_t>(cells)]);
    std::unique_ptr<uint32_t[]> w(new uint32_t[static_cast<size_t>(cells)]);
    int64_t m = -1;
    if (cells > 1) {
      std::unique_ptr<float[]> few(new float[3 * static_cast<size_t>(cells - 1)]);
      std::unique_ptr<uint32_t[]> wfew(new uint32_t[static_cast<size_t>(cells - 1)]);
      CHECK(madicp_host_cloud_export_f32_attr(xyz.get(), attr.get(), n, R, t, 1.0, few.get(), wfew.get(), cells - 1, &m) == MADICP_ERR_CAPACITY);
      CHECK(m == cells);
    }
    CHECK(madicp_host_cloud_export_f32_attr(xyz.get(), attr.get(), n, R, t, 1.0, rows.get(), w.get(), cells, &m) == MADICP_OK && m == cells);
    for (int64_t r = 0; r < cells; ++r) CHECK(w[r] == attr[2 * r] && rows[3 * r] == static_cast<float>(xyz[6 * r]));
    CHECK(madicp_host_cloud_export_f32_attr(xyz.get(), nullptr, n, R, t, 1.0, rows.get(), w.get(), cells, &m) == MADICP_ERR_INVALID);
    CHECK(madicp_host_cloud_export_f32_attr(xyz.get(), attr.get(), n, R, t, 1.0, rows.get(), nullptr, cells, &m) == MADICP_ERR_INVALID);
  }
  {  // the map: the same cloud twice with other words (the first stay), then a cloud without a column (zeros), windows of exact size
    madicp_host_map *map = nullptr, *plain = nullptr;
    CHECK(madicp_host_map_create_attr(1.0, 1, 1 << 20, &map) == MADICP_OK && madicp_host_map_create(1.0, 1, 1 << 20, &plain) == MADICP_OK);
    int64_t added = -1, rows = -1, m = -1;
    CHECK(madicp_host_map_insert_attr(map, xyz.get(), attr.get(), n, R, t, &added, &rows) == MADICP_OK && added == cells && rows == cells);
    std::unique_ptr<uint32_t[]> other(new uint32_t[static_cast<size_t>(n)]);
    for (int64_t i = 0; i < n; ++i) other[i] = 7u;
    CHECK(madicp_host_map_insert_attr(map, xyz.get(), other.get(), n, R, t, &added, &rows) == MADICP_OK && added == 0 && rows == cells);
    const double t2[3] = {0, 10, 0};
    CHECK(madicp_host_map_insert_attr(map, xyz.get(), nullptr, n, R, t2, &added, &rows) == MADICP_OK && added == cells && rows == 2 * cells);
    std::unique_ptr<uint32_t[]> w(new uint32_t[static_cast<size_t>(2 * cells)]);
    CHECK(madicp_host_map_download_attr(map, 0, w.get(), 2 * cells, &m) == MADICP_OK && m == 2 * cells);
    for (int64_t r = 0; r < cells; ++r) CHECK(w[r] == attr[2 * r] && w[cells + r] == 0u);
    std::unique_ptr<uint32_t[]> tail(new uint32_t[static_cast<size_t>(cells)]);
    CHECK(madicp_host_map_download_attr(map, cells, tail.get(), cells, &m) == MADICP_OK && m == cells);
    CHECK(madicp_host_map_download_attr(map, 0, tail.get(), cells, &m) == MADICP_ERR_CAPACITY && m == 2 * cells);
    CHECK(madicp_host_map_download_attr(map, 2 * cells + 1, tail.get(), cells, &m) == MADICP_ERR_INVALID);
    CHECK(madicp_host_map_insert(plain, xyz.get(), n, R, t, &added, &rows) == MADICP_OK);
    CHECK(madicp_host_map_download_attr(plain, 0, tail.get(), cells, &m) == MADICP_ERR_INVALID);
    CHECK(madicp_host_map_clear(map) == MADICP_OK && madicp_host_map_download_attr(map, 0, tail.get(), 0, &m) == MADICP_OK && m == 0);
    madicp_host_map_destroy(map);
    madicp_host_map_destroy(plain);
  }
  ++sets;
}

}  // namespace

int main() {
  for (int step : {13, 22, 26, 256})
    for (int type = MADICP_A_INT8; type <= MADICP_A_FLOAT32; ++type) {
      const int w = width_of(type);
      ingest_set(step, type, step - w, 1, 1);        // the field in the record's last bytes, one record per source
      ingest_set(step, type, step - w, 257, 64);     // ... the last record's field ends where the buffer does
      ingest_set(step, type, step == 13 ? 1 : 13, 31, 2);  // odd offsets: a 2- or 4-byte field straddles a dword
    }
  ingest_refusals();
  for (int64_t n : {1, 2, 65, 1025}) export_and_map_set(n);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("%d sets clean\n", sets);
  return 0;
}
