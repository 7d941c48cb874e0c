// The host twin of the device export (csrc/hip/frontend.hip.h: voxel_claim / voxel_mark / voxel_rows behind
// madicp_cloud_export_f32): a cloud out in another frame as float32, thinned to the first point of every voxel.  The per-point
// arithmetic is csrc/common/export_point.h, shared with the device kernels.  A thinned export is the first fold of the cloud into an
// empty voxel map with nothing kept afterwards — here through VoxelMap (voxel_map.h), on the device through the map's own kernels —
// so "lowest index per voxel, in index order" is stated once per side.  Header-only, like ingest_records.h: Pipeline (host front-end)
// and the C entry point madicp_host_cloud_export_f32 (cloud_export.cpp) call the one function.  Every translation unit that includes
// this is compiled without floating-point contraction.
#pragma once
#include <cstdint>

#include "../common/export_point.h"
#include "voxel_map.h"

namespace madicp_host {

constexpr int kExportOk = 0, kExportInvalid = -1, kExportCapacity = -4;  // MADICP_OK, MADICP_ERR_INVALID, MADICP_ERR_CAPACITY

// include/madicp_host.h: madicp_host_cloud_export_f32_attr — attr (n words, the cloud's column) and out_attr (the rows' words) both
// given, or both null: madicp_host_cloud_export_f32
inline int cloud_export_f32_attr(const double* xyz, const uint32_t* attr, int64_t n, const double* R, const double* t, double voxel,
                                 float* out_xyz, uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n) {
  if (!xyz || !out_xyz || !out_n || n < 0 || n > 0x3fffffff || (attr == nullptr) != (out_attr == nullptr)) return kExportInvalid;
  if (export_refusal(R, t, voxel)) return kExportInvalid;
  if (voxel == 0.0) {
    *out_n = n;
    if (capacity_rows < n) return kExportCapacity;
    for (int64_t i = 0; i < n; ++i) {
      double q[3];
      export_position(xyz + 3 * i, R, t, q);
      for (int k = 0; k < 3; ++k) out_xyz[3 * i + k] = export_value(q[k]);
      if (out_attr) out_attr[i] = attr[i];
    }
    return kExportOk;
  }
  // (the codes of VoxelMap are the export's; download sets *out_n and leaves the buffers alone on capacity)
  VoxelMap fold(voxel, n, n, out_attr != nullptr);
  int64_t added = 0, rows = 0;
  if (const int rc = fold.insert(xyz, n, R, t, &added, &rows, attr)) return rc;
  if (const int rc = fold.download(0, out_xyz, capacity_rows, out_n)) return rc;
  return out_attr ? fold.download_attr(0, out_attr, capacity_rows, out_n) : kExportOk;
}

// include/madicp_host.h: madicp_host_cloud_export_f32
inline int cloud_export_f32(const double* xyz, int64_t n, const double* R, const double* t, double voxel, float* out_xyz,
                            int64_t capacity_rows, int64_t* out_n) {
  return cloud_export_f32_attr(xyz, nullptr, n, R, t, voxel, out_xyz, nullptr, capacity_rows, out_n);
}

}  // namespace madicp_host
