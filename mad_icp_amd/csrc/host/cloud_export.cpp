// madicp_host_cloud_export_f32 (include/madicp_host.h): the C entry point of the host export (cloud_export.h).  Compiled without
// floating-point contraction, like csrc/host/deskew.cpp.
#include "cloud_export.h"

#include "madicp_host.h"

static_assert(madicp_host::kExportOk == MADICP_OK && madicp_host::kExportInvalid == MADICP_ERR_INVALID &&
                  madicp_host::kExportCapacity == MADICP_ERR_CAPACITY,
              "cloud_export.h returns the C ABI's codes");

extern "C" int madicp_host_cloud_export_f32(const double* xyz, int64_t n, const double R[9], const double t[3], double voxel,
                                            float* out_xyz, int64_t capacity_rows, int64_t* out_n) {
  return madicp_host::cloud_export_f32(xyz, n, R, t, voxel, out_xyz, capacity_rows, out_n);
}

extern "C" int madicp_host_cloud_export_f32_attr(const double* xyz, const uint32_t* attr, int64_t n, const double R[9], const double t[3],
                                                 double voxel, float* out_xyz, uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n) {
  if (!attr || !out_attr) return MADICP_ERR_INVALID;
  return madicp_host::cloud_export_f32_attr(xyz, attr, n, R, t, voxel, out_xyz, out_attr, capacity_rows, out_n);
}
