// madicp_host_map_* (include/madicp_host.h): the C entry points of the host voxel map (voxel_map.h).  Compiled without
// floating-point contraction, like everything that includes csrc/common/export_point.h.
#include "voxel_map.h"

#include <new>

#include "madicp_host.h"

static_assert(madicp_host::kMapOk == MADICP_OK && madicp_host::kMapInvalid == MADICP_ERR_INVALID &&
                  madicp_host::kMapCapacity == MADICP_ERR_CAPACITY,
              "voxel_map.h returns the C ABI's codes");

struct madicp_host_map {
  madicp_host::VoxelMap map;
};

extern "C" {

int madicp_host_map_create(double voxel, int64_t initial_rows, int64_t max_rows, madicp_host_map** out_map) {
  if (!out_map || madicp_host::map_create_refusal(voxel, initial_rows, max_rows)) return MADICP_ERR_INVALID;
  madicp_host_map* m = new (std::nothrow) madicp_host_map{madicp_host::VoxelMap(voxel, initial_rows, max_rows)};
  if (!m) return MADICP_ERR_CAPACITY;
  *out_map = m;
  return MADICP_OK;
}

int madicp_host_map_create_attr(double voxel, int64_t initial_rows, int64_t max_rows, madicp_host_map** out_map) {
  if (!out_map || madicp_host::map_create_refusal(voxel, initial_rows, max_rows)) return MADICP_ERR_INVALID;
  madicp_host_map* m = new (std::nothrow) madicp_host_map{madicp_host::VoxelMap(voxel, initial_rows, max_rows, true)};
  if (!m) return MADICP_ERR_CAPACITY;
  *out_map = m;
  return MADICP_OK;
}

int madicp_host_map_create_ev(double voxel, int64_t initial_rows, int64_t max_rows, int with_attr, uint32_t hit, uint32_t miss, uint32_t cap,
                              madicp_host_map** out_map) {
  if (!out_map || madicp_host::map_create_refusal(voxel, initial_rows, max_rows) || madicp_host::map_evidence_refusal(hit, miss, cap))
    return MADICP_ERR_INVALID;
  madicp_host_map* m =
      new (std::nothrow) madicp_host_map{madicp_host::VoxelMap(voxel, initial_rows, max_rows, with_attr != 0, true, hit, miss, cap)};
  if (!m) return MADICP_ERR_CAPACITY;
  *out_map = m;
  return MADICP_OK;
}

int madicp_host_map_create_mom(double voxel, int64_t initial_rows, int64_t max_rows, int with_attr, const uint32_t evidence[3],
                               uint32_t max_count, madicp_host_map** out_map) {
  if (!out_map || madicp_host::map_create_refusal(voxel, initial_rows, max_rows) || madicp_host::map_moments_refusal(max_count) ||
      (evidence && madicp_host::map_evidence_refusal(evidence[0], evidence[1], evidence[2])))
    return MADICP_ERR_INVALID;
  madicp_host_map* m = new (std::nothrow)
      madicp_host_map{madicp_host::VoxelMap(voxel, initial_rows, max_rows, with_attr != 0, evidence != nullptr, evidence ? evidence[0] : 1u,
                                            evidence ? evidence[1] : 1u, evidence ? evidence[2] : 1u, max_count)};
  if (!m) return MADICP_ERR_CAPACITY;
  *out_map = m;
  return MADICP_OK;
}

int madicp_host_map_download_moments(const madicp_host_map* map, int64_t first_row, uint64_t* out, int64_t capacity_rows, int64_t* out_n) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.download_moments(first_row, out, capacity_rows, out_n);
}

int madicp_host_map_download_surfels(const madicp_host_map* map, int64_t first_row, float* out_centroid, float* out_normal, float* out_eig,
                                     uint32_t* out_count, int64_t capacity_rows, int64_t* out_n) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.download_surfels(first_row, out_centroid, out_normal, out_eig, out_count, capacity_rows, out_n);
}

int madicp_host_map_download_evidence(const madicp_host_map* map, int64_t first_row, uint32_t* out_ev, int64_t capacity_rows, int64_t* out_n) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.download_evidence(first_row, out_ev, capacity_rows, out_n);
}

int madicp_host_map_download_min_evidence(const madicp_host_map* map, uint32_t min_e, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr,
                                          uint32_t* out_ev, int64_t capacity_rows, int64_t* out_n) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.download_min_evidence(min_e, out_xyz, out_keys, out_attr, out_ev, capacity_rows, out_n);
}

int madicp_host_map_insert(madicp_host_map* map, const double* xyz, int64_t n, const double R[9], const double t[3], int64_t* out_added,
                           int64_t* out_rows) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.insert(xyz, n, R, t, out_added, out_rows);
}

int madicp_host_map_insert_attr(madicp_host_map* map, const double* xyz, const uint32_t* attr, int64_t n, const double R[9],
                                const double t[3], int64_t* out_added, int64_t* out_rows) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.insert(xyz, n, R, t, out_added, out_rows, attr);
}

int madicp_host_map_merge_rows(madicp_host_map* map, double voxel, const uint64_t* keys, const float* xyz, const uint32_t* attr,
                               const uint32_t* ev, const uint64_t* mom, int64_t n, int64_t* out_added, int64_t* out_rows) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.merge_rows(voxel, keys, xyz, attr, ev, mom, n, out_added, out_rows);
}

int madicp_host_map_download_attr(const madicp_host_map* map, int64_t first_row, uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.download_attr(first_row, out_attr, capacity_rows, out_n);
}

int madicp_host_map_size(const madicp_host_map* map, int64_t* out_rows) {
  if (!map || !out_rows) return MADICP_ERR_INVALID;
  *out_rows = map->map.size();
  return MADICP_OK;
}

int madicp_host_map_download_f32(const madicp_host_map* map, int64_t first_row, float* out_xyz, int64_t capacity_rows, int64_t* out_n) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.download(first_row, out_xyz, capacity_rows, out_n);
}

int madicp_host_map_prune(madicp_host_map* map, const double center[3], double radius, int64_t watermark, int64_t* out_removed,
                          int64_t* out_rows, int64_t* out_watermark) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.prune(center, radius, watermark, out_removed, out_rows, out_watermark);
}

int madicp_host_map_clear_rays(madicp_host_map* map, const double* xyz, int64_t n, const double R[9], const double t[3],
                               const double origin[3], double margin, int64_t watermark, int64_t* out_removed, int64_t* out_rows,
                               int64_t* out_watermark) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.clearRays(xyz, n, R, t, origin, margin, watermark, out_removed, out_rows, out_watermark);
}

int madicp_host_map_track_removed(madicp_host_map* map, int on) {
  if (!map) return MADICP_ERR_INVALID;
  map->map.track_removed(on != 0);
  return MADICP_OK;
}

int madicp_host_map_removed_count(const madicp_host_map* map, int64_t* out_n) {
  if (!map || !out_n) return MADICP_ERR_INVALID;
  *out_n = map->map.removed_count();
  return MADICP_OK;
}

int madicp_host_map_take_removed(madicp_host_map* map, uint64_t* out_keys, float* out_xyz, uint32_t* out_attr, int64_t capacity,
                                 int64_t* out_n) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.take_removed(out_keys, out_xyz, out_attr, capacity, out_n);
}

int madicp_host_map_download_keys(const madicp_host_map* map, int64_t first_row, uint64_t* out_keys, int64_t capacity_rows, int64_t* out_n) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.download_keys(first_row, out_keys, capacity_rows, out_n);
}

int madicp_host_map_download_rows(const madicp_host_map* map, int64_t first_row, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr,
                                  int64_t capacity_rows, int64_t* out_n) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.download_rows(first_row, out_xyz, out_keys, out_attr, capacity_rows, out_n);
}

int madicp_host_map_query(const madicp_host_map* map, const double* xyz, int64_t n, const double R[9], const double t[3], int reach,
                          double max_dist, int32_t* out_row, double* out_d2, uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev,
                          int64_t capacity_points, uint64_t out_counts[3]) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.query(xyz, n, R, t, reach, max_dist, out_row, out_d2, out_keys, out_attr, out_ev, capacity_points, out_counts);
}

int madicp_host_map_score(const madicp_host_map* map, const double* xyz, int64_t n, const double* poses, int64_t n_poses, int reach,
                          double max_dist, int64_t stride, uint64_t* out_counts) {
  if (!map) return MADICP_ERR_INVALID;
  return map->map.score(xyz, n, poses, n_poses, reach, max_dist, stride, out_counts);
}

int madicp_host_map_register(const madicp_host_map* map, const double* xyz, int64_t n, const double R[9], const double t[3],
                             const madicp_map_align_params* params, int iterations, double out_R[9], double out_t[3],
                             double* out_trace, uint64_t* out_counts, int32_t* out_row, double* out_e, int64_t capacity_points) {
  if (!map || !params) return MADICP_ERR_INVALID;
  return map->map.align(xyz, n, R, t, params->reach, params->max_dist, params->rho, params->min_count, params->flat, iterations, out_R,
                        out_t, out_trace, out_counts, out_row, out_e, capacity_points);
}

int madicp_host_map_clear(madicp_host_map* map) {
  if (!map) return MADICP_ERR_INVALID;
  map->map.clear();
  return MADICP_OK;
}

void madicp_host_map_destroy(madicp_host_map* map) { delete map; }

}  // extern "C"
