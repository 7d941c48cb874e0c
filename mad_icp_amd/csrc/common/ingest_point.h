// What happens to ONE sensor record on its way into a cloud — ONE source for the device ingest kernels (csrc/hip/frontend.hip.h:
// ingest_mark / ingest_scatter on float32 rows, sources_mark / sources_scatter on byte records) and for the host twin
// (csrc/host/ingest_records.cpp), so the three cannot drift apart: the range filter of apps/cpp_runners/bin_runner.cpp:149-151,
// the "kitti magic correction" of :153-158, and the normalisation of a record's time field.  Every translation unit that
// includes this is compiled WITHOUT floating-point contraction (-ffp-contract=off; the device header adds the pragma).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "eig3.h"  // MADICP_HD, sum3c, sum3s

namespace madicp_host {

// the record is DROPPED: |p| < min_range or |p| > max_range or a NaN coordinate; |p| evaluated in float like
// Eigen::Vector3f::norm() (squares summed as x^2 + (y^2 + z^2): the unrolled scalar reduction of a 3-vector, no packet for three
// floats), compared in double.  ON a bound stays.
MADICP_HD inline bool ingest_drops(float x, float y, float z, double min_range, double max_range) {
  const float nrm = sqrtf(x * x + (y * y + z * z));
  return (double)nrm < min_range || (double)nrm > max_range || x != x || y != y || z != z;
}

// float coordinates -> the cloud's doubles; kitti: rotate the point by VERTICAL_ANGLE_OFFSET about the normalised p x (0,0,1).
// sin / cos of the constant angle come from the caller (host libm).  The rotation is Eigen's AngleAxisd::toRotationMatrix()
// followed by a 3x3 * vector product.
MADICP_HD inline void ingest_point(float xf, float yf, float zf, int kitti, double sin_a, double cos_a, double* o) {
  const double x = (double)xf, y = (double)yf, z = (double)zf;
  double o0 = x, o1 = y, o2 = z;
  if (kitti) {
    // rotation_vector = p.cross((0,0,1)) = (y*1 - z*0, z*0 - x*1, x*0 - y*0)
    const double r0 = y * 1.0 - z * 0.0, r1 = z * 0.0 - x * 1.0, r2 = x * 0.0 - y * 0.0;
    double a0 = r0, a1 = r1, a2 = r2;
    const double sq = sum3c(r0 * r0, r1 * r1, r2 * r2);  // squaredNorm of a contiguous Vector3d
    if (sq > 0.0) {  // Eigen's normalized(): left alone when the squared norm is not positive
      const double nn = sqrt(sq);
      a0 = r0 / nn; a1 = r1 / nn; a2 = r2 / nn;
    }
    const double s0 = sin_a * a0, s1 = sin_a * a1, s2 = sin_a * a2;
    const double c1_0 = (1.0 - cos_a) * a0, c1_1 = (1.0 - cos_a) * a1, c1_2 = (1.0 - cos_a) * a2;
    double R[9];
    double tmp = c1_0 * a1;
    R[1] = tmp - s2; R[3] = tmp + s2;
    tmp = c1_0 * a2;
    R[2] = tmp + s1; R[6] = tmp - s1;
    tmp = c1_1 * a2;
    R[5] = tmp - s0; R[7] = tmp + s0;
    R[0] = c1_0 * a0 + cos_a; R[4] = c1_1 * a1 + cos_a; R[8] = c1_2 * a2 + cos_a;
    o0 = sum3s(R[0] * x, R[1] * y, R[2] * z);
    o1 = sum3s(R[3] * x, R[4] * y, R[5] * z);
    o2 = sum3s(R[6] * x, R[7] * y, R[8] * z);
  }
  o[0] = o0; o[1] = o1; o[2] = o2;
}
// VERTICAL_ANGLE_OFFSET = (0.205 * M_PI) / 180.0 (bin_runner.cpp:55)
inline double ingest_kitti_angle() { return (0.205 * M_PI) / 180.0; }

// ---- byte records (include/madicp_hip.h: madicp_record_layout) ------------------------------------------------------------------
// The fields of a record sit at ANY alignment (a packed 22-byte XYZIRT record, a float64 time at offset 18): they are read
// byte-wise through memcpy, never through a cast of the address.  Little-endian, like the machine.
constexpr int kTimeNone = 0, kTimeU32 = 6, kTimeF32 = 7, kTimeF64 = 8;  // sensor_msgs/PointField's codes (MADICP_T_*)
constexpr int kRecordStepMin = 12, kRecordStepMax = 256;

struct RecordLayout {  // madicp_record_layout, validated (record_layout_ok)
  int32_t step, off_x, off_y, off_z, off_t, t_type;
};

inline bool record_layout_ok(const RecordLayout& L) {
  if (L.step < kRecordStepMin || L.step > kRecordStepMax) return false;
  const int32_t offs[3] = {L.off_x, L.off_y, L.off_z};
  for (int32_t o : offs)
    if (o < 0 || o > L.step - 4) return false;
  if (L.t_type == kTimeNone) return true;
  if (L.t_type != kTimeU32 && L.t_type != kTimeF32 && L.t_type != kTimeF64) return false;
  const int32_t width = L.t_type == kTimeF64 ? 8 : 4;
  return L.off_t >= 0 && L.off_t <= L.step - width;
}

MADICP_HD inline float record_f32(const unsigned char* p) {
  float v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
// the time of a record as a double: exact for all three field types
MADICP_HD inline double record_time(const unsigned char* p, int t_type) {
  if (t_type == kTimeF64) {
    double v;
    __builtin_memcpy(&v, p, 8);
    return v;
  }
  if (t_type == kTimeF32) return (double)record_f32(p);
  uint32_t u;
  __builtin_memcpy(&u, p, 4);
  return (double)u;
}
MADICP_HD inline bool time_is_finite(double t) { return t - t == 0.0; }  // (inf - inf and NaN - NaN are NaN)

// ---- the attribute: ONE more field of the record (intensity, reflectivity, ring, a label ...) carried beside the point as a 32-bit
// word — the field's bytes, little-endian, zero-extended.  Nothing converts, scales or interprets it: an INT16 of -1 is the word
// 0x0000ffff, a FLOAT32 keeps its bits (NaN payloads and -0.0 included).  Types are sensor_msgs/PointField's codes (MADICP_A_*).
constexpr int kAttrNone = 0, kAttrI8 = 1, kAttrU8 = 2, kAttrI16 = 3, kAttrU16 = 4, kAttrI32 = 5, kAttrU32 = 6, kAttrF32 = 7;
struct AttrField {  // madicp_attr_field
  int32_t off, type;
};
MADICP_HD inline int attr_width(int type) { return type <= kAttrU8 ? 1 : (type <= kAttrU16 ? 2 : 4); }
MADICP_HD inline uint32_t record_attr(const unsigned char* p, int type) {
  uint32_t w = 0;
  if (type <= kAttrU8) __builtin_memcpy(&w, p, 1);
  else if (type <= kAttrU16) __builtin_memcpy(&w, p, 2);
  else __builtin_memcpy(&w, p, 4);
  return w;
}
// the field lies inside the record and its type is known
inline bool attr_field_ok(const RecordLayout& L, const AttrField& A) {
  if (A.type < kAttrI8 || A.type > kAttrF32) return false;
  return A.off >= 0 && A.off <= L.step - attr_width(A.type);
}

// the stamp of a record, normalised over [t0, t1]: NaN unless the span is positive (all times equal, or no finite time at all);
// +-inf and values outside [0, 1] are left as IEEE produces them — stamp_chunk() clamps them
MADICP_HD inline double record_stamp(double t64, double t0, double t1) {
  const double span = t1 - t0;
  if (!(span > 0.0)) return std::numeric_limits<double>::quiet_NaN();
  return (t64 - t0) / span;
}

// ---- several sources into one cloud (include/madicp_hip.h: madicp_record_source) ------------------------------------------------
// the time of a record on the clock all sources share: tc = t64 * t_scale + t_offset, two roundings (no fma: these translation
// units are compiled without contraction).  `as_is`: the host found t_scale == 1.0 and t_offset == 0.0 exactly — the time is
// taken unchanged (x * 1.0 + 0.0 would turn a -0.0 into +0.0), so that a plain source (plain_source) keeps its times bit for bit.
MADICP_HD inline double source_clock(double t64, int as_is, double t_scale, double t_offset) {
  if (as_is) return t64;
  const double scaled = t64 * t_scale;
  return scaled + t_offset;
}
inline bool source_clock_as_is(double t_scale, double t_offset) { return t_scale == 1.0 && t_offset == 0.0; }

// sensor frame -> base frame, AFTER ingest_point (the KITTI rotation belongs to the sensor frame): R row-major, the evaluation
// order of pose * point in the stamped deskew (fe::deskew_stamped / deskew_cloud_stamped), both of its branches.  In place.
MADICP_HD inline void sensor_to_base(const double* R, const double* t, double* o) {
  const double x = o[0], y = o[1], z = o[2];
#ifdef MADICP_XFORM_HOMOGENEOUS
  o[0] = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
  o[1] = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
  o[2] = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
#else
  o[0] = t[0] + sum3s(R[0] * x, R[1] * y, R[2] * z);
  o[1] = t[1] + sum3s(R[3] * x, R[4] * y, R[5] * z);
  o[2] = t[2] + sum3s(R[6] * x, R[7] * y, R[8] * z);
#endif
}
// a source whose extrinsic is exactly the identity skips sensor_to_base (0.0 + (x + (0.0 + 0.0)) would lose the sign of a zero)
inline bool source_extrinsic_is_identity(const double* R, const double* t) {
  for (int i = 0; i < 9; ++i)
    if (R[i] != ((i % 4 == 0) ? 1.0 : 0.0)) return false;
  return t[0] == 0.0 && t[1] == 0.0 && t[2] == 0.0;
}

constexpr int kMaxSources = 8;  // MADICP_MAX_SOURCES
struct RecordSource {           // madicp_record_source with its layout as a RecordLayout
  const void* data;
  int64_t n;
  RecordLayout L;
  double R[9], t[3];
  double min_range, max_range;
  double t_scale, t_offset;
  int32_t kitti;
  AttrField A;  // the attribute field; type kAttrNone (what value-initialisation leaves): none is carried
};
// (from the C ABI's madicp_record_source: a template, so that this header needs none of the C headers)
template <class CSource>
inline RecordSource record_source_of(const CSource& c) {
  RecordSource S;
  S.data = c.data;
  S.n = c.n_records;
  S.L = RecordLayout{c.layout.point_step, c.layout.off_x, c.layout.off_y, c.layout.off_z, c.layout.off_t, c.layout.t_type};
  for (int i = 0; i < 9; ++i) S.R[i] = c.R[i];
  for (int i = 0; i < 3; ++i) S.t[i] = c.t[i];
  S.min_range = c.min_range;
  S.max_range = c.max_range;
  S.t_scale = c.t_scale;
  S.t_offset = c.t_offset;
  S.kitti = c.kitti_correction;
  S.A = AttrField{0, kAttrNone};  // (the C struct has none: madicp_cloud_ingest_sources_attr passes the fields beside the sources)
  return S;
}
// (and back)
template <class CSource>
inline CSource record_source_to(const RecordSource& S) {
  CSource c{};
  c.data = S.data;
  c.n_records = S.n;
  c.layout = {S.L.step, S.L.off_x, S.L.off_y, S.L.off_z, S.L.off_t, S.L.t_type};
  for (int i = 0; i < 9; ++i) c.R[i] = S.R[i];
  for (int i = 0; i < 3; ++i) c.t[i] = S.t[i];
  c.min_range = S.min_range;
  c.max_range = S.max_range;
  c.t_scale = S.t_scale;
  c.t_offset = S.t_offset;
  c.kitti_correction = S.kitti ? 1 : 0;
  return c;
}
// The PLAIN source: one sensor already in the base frame and on the common clock — the identity extrinsic (sensor_to_base is
// skipped), t_scale 1 and t_offset 0 (source_clock takes the time as it is).  The single-source ingests of every layer
// (madicp_cloud_ingest_records, ingest_records, Pipeline::computeRecordsStamped) are the sources ingest of this one source.
inline RecordSource plain_source(const void* data, int64_t n, const RecordLayout& L, double min_range, double max_range, bool kitti) {
  return RecordSource{data, n, L, {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}, min_range, max_range, 1.0, 0.0, kitti ? 1 : 0,
                      AttrField{0, kAttrNone}};
}

// what every layer refuses before it touches a record (null = nothing to refuse): the device entry, the host twin and Pipeline
// ask this one function
inline const char* record_sources_refusal(const RecordSource* src, int n_sources, const double* t_range) {
  if (!src) return "null argument";
  if (n_sources < 1 || n_sources > kMaxSources) return "1 .. 8 sources";
  int64_t total = 0;
  for (int s = 0; s < n_sources; ++s) {
    const RecordSource& S = src[s];
    if (!S.data) return "null argument";
    if (S.n < 1 || S.n > 0x40000000) return "every source holds at least one record, all of them together at most 2^30";
    total += S.n;
    if (!record_layout_ok(S.L)) return "record layout: point_step 12 .. 256, every field inside the record, t_type one of MADICP_T_*";
    for (double v : S.R)
      if (!time_is_finite(v)) return "R and t: finite entries";
    for (double v : S.t)
      if (!time_is_finite(v)) return "R and t: finite entries";
    if (!time_is_finite(S.t_scale) || !(S.t_scale > 0.0) || !time_is_finite(S.t_offset)) return "t_scale finite and > 0, t_offset finite";
    if ((S.L.t_type != kTimeNone) != (src[0].L.t_type != kTimeNone)) return "a time field in every source or in none";
    if (S.A.type != kAttrNone && !attr_field_ok(S.L, S.A)) return "attribute field: inside the record, type one of MADICP_A_*";
    if ((S.A.type != kAttrNone) != (src[0].A.type != kAttrNone)) return "an attribute in every source or in none";
    if (S.A.type != src[0].A.type) return "the same attribute type in every source";
  }
  if (total > 0x40000000) return "every source holds at least one record, all of them together at most 2^30";
  if (t_range && !(time_is_finite(t_range[0]) && time_is_finite(t_range[1]) && t_range[1] > t_range[0]))
    return "t_range: both values finite, t_end > t_begin";
  return nullptr;
}

}  // namespace madicp_host
