// The host twins of madicp_cloud_ingest_sources and madicp_cloud_ingest_records (include/madicp_hip.h; kernels in
// csrc/hip/frontend.hip.h): drivers' byte records — any record step, float32 x / y / z and a uint32 / float32 / float64 time
// field at any alignment — to the range-filtered points in input order and their stamps normalised over the scan.  ONE loop nest,
// ingest_sources; a single buffer of records is its one plain source (ingest_records).  The per-record arithmetic is
// csrc/common/ingest_point.h, the one source the device kernels use as well, and this file is compiled without floating-point
// contraction like csrc/host/deskew.cpp: bit-equal to the device by construction.  Every field is read through memcpy; nothing
// past data[n * step) is touched.  What a Pipeline with the host front-end runs for computeRecordsStamped / computeSourcesStamped.
// Defined inline here, so that every program that compiles pipeline.cpp has it whatever else it links; ingest_records.cpp holds
// the exported C entry points (madicp_host_ingest_records, madicp_host_ingest_sources: include/madicp_host.h).
#pragma once
#include <cmath>
#include <cstdint>

#include "../common/ingest_point.h"

namespace madicp_host {

// The host twin of madicp_cloud_ingest_sources: several sources' records -> one base-frame cloud, source 0's survivors first in
// input order, then source 1's ..., with one set of stamps normalised on the common clock (ingest_point.h: source_clock,
// sensor_to_base; the range filter in each sensor's own frame with its own bounds).  out_xyz: room for (total records, 3)
// doubles, out_stamps01: room for that many (may be null; not written without a time field); out_n_per_source (n_sources
// values) and out_t_range: optional.  t_range: null = min / max of the finite times of ALL records on the common clock, dropped
// ones included, each canonicalised as t + 0.0; else {t_begin, t_end}.  out_t_range: the range used (+inf, -inf without a time
// field or a finite time).  Returns 0; -1 for what record_sources_refusal refuses or a null out_xyz / out_n, nothing
// written.  No survivor is NOT an error here: *out_n = 0.  Nothing past data[n * step) of any source is touched.
// ingest_sources_attr — the twin of madicp_cloud_ingest_sources_attr — is the loop nest: sources that name an attribute field
// (RecordSource::A, all or none) leave every survivor's word (ingest_point.h: record_attr) in out_attr, room for one per record;
// -1 as well for a null out_attr with such sources.  ingest_sources is the same call for sources that name none.
inline int ingest_sources_attr(const RecordSource* src, int n_sources, const double* t_range, double* out_xyz, double* out_stamps01,
                               uint32_t* out_attr, int64_t* out_n, int64_t* out_n_per_source, double* out_t_range) {
  if (!out_xyz || !out_n) return -1;
  if (record_sources_refusal(src, n_sources, t_range)) return -1;
  const bool has_attr = src[0].A.type != kAttrNone;
  if (has_attr && !out_attr) return -1;
  const bool has_time = src[0].L.t_type != kTimeNone;
  bool as_is[kMaxSources];
  for (int s = 0; s < n_sources; ++s) as_is[s] = source_clock_as_is(src[s].t_scale, src[s].t_offset);
  // the range: every record of every source, dropped ones included, finite times on the common clock only
  double t0 = HUGE_VAL, t1 = -HUGE_VAL;
  if (has_time && t_range) {
    t0 = t_range[0];
    t1 = t_range[1];
  } else if (has_time) {
    for (int s = 0; s < n_sources; ++s) {
      const RecordSource& S = src[s];
      const unsigned char* rec = static_cast<const unsigned char*>(S.data);
      for (int64_t i = 0; i < S.n; ++i) {
        const double tc = source_clock(record_time(rec + i * S.L.step + S.L.off_t, S.L.t_type), as_is[s] ? 1 : 0, S.t_scale, S.t_offset);
        if (!time_is_finite(tc)) continue;
        if (tc < t0) t0 = tc;
        if (tc > t1) t1 = tc;
      }
    }
    t0 = t0 + 0.0;  // (a -0.0 extreme becomes +0.0)
    t1 = t1 + 0.0;
  }
  const double angle = ingest_kitti_angle();
  const double sin_a = std::sin(angle), cos_a = std::cos(angle);
  int64_t kept = 0;
  for (int s = 0; s < n_sources; ++s) {
    const RecordSource& S = src[s];
    const RecordLayout& L = S.L;
    const unsigned char* rec = static_cast<const unsigned char*>(S.data);
    const bool identity = source_extrinsic_is_identity(S.R, S.t);
    const int64_t before = kept;
    for (int64_t i = 0; i < S.n; ++i) {
      const unsigned char* p = rec + i * L.step;
      const float x = record_f32(p + L.off_x), y = record_f32(p + L.off_y), z = record_f32(p + L.off_z);
      if (ingest_drops(x, y, z, S.min_range, S.max_range)) continue;
      double* o = out_xyz + 3 * kept;
      ingest_point(x, y, z, S.kitti ? 1 : 0, sin_a, cos_a, o);
      if (!identity) sensor_to_base(S.R, S.t, o);
      if (has_time && out_stamps01)
        out_stamps01[kept] = record_stamp(source_clock(record_time(p + L.off_t, L.t_type), as_is[s] ? 1 : 0, S.t_scale, S.t_offset), t0, t1);
      if (has_attr) out_attr[kept] = record_attr(p + S.A.off, S.A.type);
      ++kept;
    }
    if (out_n_per_source) out_n_per_source[s] = kept - before;
  }
  *out_n = kept;
  if (out_t_range) {
    out_t_range[0] = t0;
    out_t_range[1] = t1;
  }
  return 0;
}

inline int ingest_sources(const RecordSource* src, int n_sources, const double* t_range, double* out_xyz, double* out_stamps01,
                          int64_t* out_n, int64_t* out_n_per_source, double* out_t_range) {
  return ingest_sources_attr(src, n_sources, t_range, out_xyz, out_stamps01, nullptr, out_n, out_n_per_source, out_t_range);
}

// ... and of madicp_cloud_ingest_records: ingest_sources of the one plain source (ingest_point.h: plain_source), so out_xyz has
// room for (n, 3) doubles, out_stamps01 for n.  Returns 0; -1 on bad arguments (a null pointer, n outside 1 .. 2^30 - 1 — the
// bound of its own that this entry keeps —, a layout record_layout_ok refuses, a t_range that is not finite and increasing),
// nothing written.
inline int ingest_records(const void* data, int64_t n, const RecordLayout& L, double min_range, double max_range, bool kitti_correction,
                          const double* t_range, double* out_xyz, double* out_stamps01, int64_t* out_n, double* out_t_range) {
  if (n > 0x3fffffff) return -1;
  const RecordSource S = plain_source(data, n, L, min_range, max_range, kitti_correction);
  return ingest_sources(&S, 1, t_range, out_xyz, out_stamps01, out_n, nullptr, out_t_range);
}

}  // namespace madicp_host
