// The host twin of the device export (csrc/hip/frontend.hip.h: export_claim / export_mark / export_scatter): a cloud out in
// another frame as float32, thinned to the first point of every voxel.  The per-point arithmetic is csrc/common/export_point.h,
// shared with the device kernels; "lowest index per voxel" is a sort of (key, index) pairs here, a hash table there — the result
// is a function of the input alone either way.  Header-only, like ingest_records.h: Pipeline (host front-end) and the C entry point
// madicp_host_cloud_export_f32 (cloud_export.cpp) call the one function.  Every translation unit that includes this is compiled
// without floating-point contraction.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../common/export_point.h"

namespace madicp_host {

constexpr int kExportOk = 0, kExportInvalid = -1, kExportCapacity = -4;  // MADICP_OK, MADICP_ERR_INVALID, MADICP_ERR_CAPACITY

// include/madicp_host.h: madicp_host_cloud_export_f32
inline int cloud_export_f32(const double* xyz, int64_t n, const double* R, const double* t, double voxel, float* out_xyz,
                            int64_t capacity_rows, int64_t* out_n) {
  if (!xyz || !out_xyz || !out_n || n < 0 || n > 0x3fffffff) return kExportInvalid;
  if (export_refusal(R, t, voxel)) return kExportInvalid;
  auto emit = [&](int64_t i, int64_t row) {
    double q[3];
    export_position(xyz + 3 * i, R, t, q);
    for (int k = 0; k < 3; ++k) out_xyz[3 * row + k] = export_value(q[k]);
  };
  if (voxel == 0.0) {
    *out_n = n;
    if (capacity_rows < n) return kExportCapacity;
    for (int64_t i = 0; i < n; ++i) emit(i, i);
    return kExportOk;
  }
  // the candidates as (key, index), sorted: the first of every run of equal keys is the voxel's lowest index
  std::vector<std::pair<uint64_t, uint32_t>> cand;
  cand.reserve(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    double q[3];
    export_position(xyz + 3 * i, R, t, q);
    const uint64_t key = export_key(q, voxel);
    if (key != kExportNoKey) cand.emplace_back(key, static_cast<uint32_t>(i));
  }
  std::sort(cand.begin(), cand.end());
  std::vector<uint32_t> kept;
  for (size_t c = 0; c < cand.size(); ++c)
    if (c == 0 || cand[c].first != cand[c - 1].first) kept.push_back(cand[c].second);
  std::sort(kept.begin(), kept.end());
  const int64_t m = static_cast<int64_t>(kept.size());
  *out_n = m;
  if (capacity_rows < m) return kExportCapacity;
  for (int64_t row = 0; row < m; ++row) emit(kept[static_cast<size_t>(row)], row);
  return kExportOk;
}

}  // namespace madicp_host
