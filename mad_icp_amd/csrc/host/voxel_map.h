// The host twin of the device voxel map (csrc/hip/frontend.hip.h: voxel_claim / voxel_mark / voxel_rows / map_rehash): an append-only
// set of float32 rows, one per voxel, the first point ever to fall into a voxel.  The per-point arithmetic is
// csrc/common/export_point.h, shared with the device kernels and the export — the KEY comes from the fp64 position, never from the
// float that is stored.  "Lowest index of the new points of a key" is the order of one sequential pass here, two integer atomics
// behind a kernel boundary there: the map is a function of the sequence of (cloud, pose) alone either way.  Header-only, like
// ingest_records.h: Pipeline (host front-end), the C entry points madicp_host_map_* (voxel_map.cpp) and the thinned export
// (cloud_export.h: one fold into a temporary map) use the one class.  Every translation unit that includes this is compiled without
// floating-point contraction.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <unordered_set>
#include <vector>

#include "../common/export_point.h"

namespace madicp_host {

constexpr int kMapOk = 0, kMapInvalid = -1, kMapCapacity = -4;  // MADICP_OK, MADICP_ERR_INVALID, MADICP_ERR_CAPACITY

class VoxelMap {
 public:
  VoxelMap(double voxel, int64_t initial_rows, int64_t max_rows) : voxel_(voxel), max_rows_(max_rows) {
    const size_t first = static_cast<size_t>(std::min(initial_rows, max_rows));
    rows_.reserve(3 * first);
    keys_.reserve(first);
  }
  double voxel() const { return voxel_; }
  int64_t size() const { return static_cast<int64_t>(rows_.size() / 3); }

  // include/madicp_host.h: madicp_host_map_insert
  int insert(const double* xyz, int64_t n, const double* R, const double* t, int64_t* out_added, int64_t* out_rows) {
    if (!out_added || !out_rows || n < 0 || n > kMapMaxRows || (!xyz && n > 0)) return kMapInvalid;
    if (export_refusal(R, t, voxel_)) return kMapInvalid;
    if (size() + n > max_rows_) return kMapCapacity;  // (conservative: decided before a point is looked at, as on the device)
    const int64_t before = size();
    for (int64_t i = 0; i < n; ++i) {
      double q[3];
      export_position(xyz + 3 * i, R, t, q);
      const uint64_t key = export_key(q, voxel_);
      if (key == kExportNoKey || !keys_.insert(key).second) continue;
      for (int k = 0; k < 3; ++k) rows_.push_back(export_value(q[k]));
    }
    *out_added = size() - before;
    *out_rows = size();
    return kMapOk;
  }

  // include/madicp_host.h: madicp_host_map_download_f32 — rows [first_row, size())
  int download(int64_t first_row, float* out, int64_t capacity_rows, int64_t* out_n) const {
    if (!out || !out_n || first_row < 0 || first_row > size()) return kMapInvalid;
    const int64_t m = size() - first_row;
    *out_n = m;
    if (capacity_rows < m) return kMapCapacity;
    if (m > 0) std::memcpy(out, rows_.data() + 3 * first_row, sizeof(float) * 3 * static_cast<size_t>(m));
    return kMapOk;
  }

  void clear() {  // (keeps the memory, forgets the rows)
    rows_.clear();
    keys_.clear();
  }

 private:
  double voxel_;
  int64_t max_rows_;
  std::vector<float> rows_;
  std::unordered_set<uint64_t> keys_;
};

}  // namespace madicp_host
