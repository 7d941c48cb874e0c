// madicp_host_ingest_records, madicp_host_ingest_sources, madicp_host_ingest_sources_attr (include/madicp_host.h): the C entry points of the host records ingest
// (ingest_records.h).  Compiled without floating-point contraction, like csrc/host/deskew.cpp.
#include "ingest_records.h"

#include "madicp_host.h"

extern "C" int madicp_host_ingest_records(const void* data, int64_t n_records, const madicp_record_layout* layout, double min_range,
                                          double max_range, int kitti_correction, const double* t_range, double* out_xyz,
                                          double* out_stamps01, int64_t* out_n, double out_t_range[2]) {
  if (!layout) return -1;
  const madicp_host::RecordLayout L{layout->point_step, layout->off_x, layout->off_y, layout->off_z, layout->off_t, layout->t_type};
  return madicp_host::ingest_records(data, n_records, L, min_range, max_range, kitti_correction != 0, t_range, out_xyz, out_stamps01,
                                     out_n, out_t_range);
}

extern "C" int madicp_host_ingest_sources(const madicp_record_source* sources, int n_sources, const double* t_range, double* out_xyz,
                                          double* out_stamps01, int64_t* out_n, int64_t* out_n_per_source, double out_t_range[2]) {
  if (!sources || n_sources < 1 || n_sources > MADICP_MAX_SOURCES) return -1;
  madicp_host::RecordSource src[MADICP_MAX_SOURCES];
  for (int s = 0; s < n_sources; ++s) src[s] = madicp_host::record_source_of(sources[s]);
  return madicp_host::ingest_sources(src, n_sources, t_range, out_xyz, out_stamps01, out_n, out_n_per_source, out_t_range);
}

extern "C" int madicp_host_ingest_sources_attr(const madicp_record_source* sources, int n_sources, const madicp_attr_field* fields,
                                               const double* t_range, double* out_xyz, double* out_stamps01, uint32_t* out_attr,
                                               int64_t* out_n, int64_t* out_n_per_source, double out_t_range[2]) {
  if (!sources || n_sources < 1 || n_sources > MADICP_MAX_SOURCES) return -1;
  madicp_host::RecordSource src[MADICP_MAX_SOURCES];
  for (int s = 0; s < n_sources; ++s) {
    src[s] = madicp_host::record_source_of(sources[s]);
    if (fields) src[s].A = madicp_host::AttrField{fields[s].offset, fields[s].type};
  }
  return madicp_host::ingest_sources_attr(src, n_sources, t_range, out_xyz, out_stamps01, out_attr, out_n, out_n_per_source, out_t_range);
}
