"""The layout of a driver's point records, read off a numpy dtype.

A LiDAR driver delivers a PointCloud2-style byte buffer: records `point_step` bytes apart, float32 x / y / z at byte offsets and
— usually — a per-point time field named `t`, `timestamp` or `time` (uint32 nanoseconds, float32 or float64 seconds).  A reader
such as the reference's apps/utils/point_cloud2.py::read_points returns it as a 1-D numpy STRUCTURED array; this module turns
that array's dtype into the six integers of madicp_record_layout (include/madicp_hip.h), which is all the native layers take:

    layout_of(dtype, time_field=None) -> RecordLayout(point_step, off_x, off_y, off_z, off_t, t_type)
    resolve(records, time_field=None, layout=None) -> (n_records, RecordLayout)     what Pipeline.computeRecordsStamped calls

and, for a rig of several sensors (Pipeline.computeSourcesStamped, madicp_cloud_ingest_sources):

    Source(records, min_range, max_range, sensor_to_base=None, time_scale=1.0, time_offset=0.0, kitti_correction=False,
           time_field=None, layout=None)                                           one sensor's buffer and how to read it
    resolve_sources(sources) -> [ResolvedSource(...)]                              what Pipeline.computeSourcesStamped calls

and, for a per-point ATTRIBUTE carried from the records to the exported scan and the map (one more field of the record — intensity,
reflectivity, ring, a label — as a 32-bit word per point, its bytes zero-extended, never converted):

    attribute_of(dtype, name) -> (offset, type code A_*, numpy dtype)               the field as madicp_attr_field takes it
    attribute_view(words, dtype) -> the uint32 words viewed back as the field's dtype

`time_field=None` takes the first of `t`, `timestamp`, `time` that the dtype has (point_cloud2.py:72), and no time field at
all (t_type = T_NONE) when it has none; `time_field=False` ignores a time field that is there.
"""
import collections
import sys

import numpy as np

T_NONE, T_U32, T_F32, T_F64 = 0, 6, 7, 8  # sensor_msgs/PointField's own codes (MADICP_T_*)
TIME_FIELD_NAMES = ("t", "timestamp", "time")
POINT_STEP_MIN, POINT_STEP_MAX = 12, 256

RecordLayout = collections.namedtuple("RecordLayout", "point_step off_x off_y off_z off_t t_type")

_TIME_TYPES = {("u", 4): T_U32, ("f", 4): T_F32, ("f", 8): T_F64}
_TIME_WIDTH = {T_U32: 4, T_F32: 4, T_F64: 8}


def _little_endian(dt):
    return dt.byteorder == "<" or dt.byteorder == "|" or (dt.byteorder == "=" and sys.byteorder == "little")


def layout_of(dtype, time_field=None):
    """RecordLayout of a structured dtype.  ValueError for: no fields, an itemsize outside 12 .. 256, a missing or non-float32 or
    big-endian x / y / z, a named time field that is missing, a time field that is big-endian or not uint32 / float32 / float64."""
    dtype = np.dtype(dtype)
    if dtype.fields is None:
        raise ValueError("a structured dtype with fields x, y, z is needed, got %r" % (dtype,))
    if not POINT_STEP_MIN <= dtype.itemsize <= POINT_STEP_MAX:
        raise ValueError("itemsize (point_step) %d outside %d .. %d" % (dtype.itemsize, POINT_STEP_MIN, POINT_STEP_MAX))
    offs = []
    for name in ("x", "y", "z"):
        if name not in dtype.fields:
            raise ValueError("the records have no field %r" % name)
        dt, off = dtype.fields[name][:2]
        if dt.shape != () or dt.kind != "f" or dt.itemsize != 4:
            raise ValueError("field %r must be float32, is %r" % (name, dt))
        if not _little_endian(dt):
            raise ValueError("field %r is big-endian: little-endian records only" % name)
        offs.append(int(off))
    if time_field is None:
        time_field = next((n for n in TIME_FIELD_NAMES if n in dtype.fields), False)
    if time_field is False:
        return RecordLayout(dtype.itemsize, offs[0], offs[1], offs[2], 0, T_NONE)
    if time_field not in dtype.fields:
        raise ValueError("the records have no time field %r" % (time_field,))
    dt, off = dtype.fields[time_field][:2]
    t_type = _TIME_TYPES.get((dt.kind, dt.itemsize)) if dt.shape == () else None
    if t_type is None:
        raise ValueError("time field %r: unsupported dtype %r (uint32, float32 or float64)" % (time_field, dt))
    if not _little_endian(dt):
        raise ValueError("time field %r is big-endian: little-endian records only" % (time_field,))
    return RecordLayout(dtype.itemsize, offs[0], offs[1], offs[2], int(off), t_type)


A_NONE, A_INT8, A_UINT8, A_INT16, A_UINT16, A_INT32, A_UINT32, A_FLOAT32 = range(8)  # sensor_msgs/PointField's codes (MADICP_A_*)
_ATTR_TYPES = {("i", 1): A_INT8, ("u", 1): A_UINT8, ("i", 2): A_INT16, ("u", 2): A_UINT16, ("i", 4): A_INT32, ("u", 4): A_UINT32,
               ("f", 4): A_FLOAT32}
ATTR_DTYPE = {code: np.dtype("<" + kind + str(size)) for (kind, size), code in _ATTR_TYPES.items()}


def attribute_of(dtype, name):
    """(byte offset, type code, little-endian numpy dtype) of the field `name` of a structured dtype: what the native layers take as
    a madicp_attr_field, and what the words they return are viewed back as.  ValueError for: no fields, a missing field, a
    big-endian one, a dtype that is not int8 / uint8 / int16 / uint16 / int32 / uint32 / float32."""
    dtype = np.dtype(dtype)
    if dtype.fields is None:
        raise ValueError("a structured dtype is needed to name an attribute field, got %r" % (dtype,))
    if name not in dtype.fields:
        raise ValueError("the records have no attribute field %r" % (name,))
    dt, off = dtype.fields[name][:2]
    code = _ATTR_TYPES.get((dt.kind, dt.itemsize)) if dt.shape == () else None
    if code is None:
        raise ValueError("attribute field %r: unsupported dtype %r (int8 .. uint32 or float32)" % (name, dt))
    if not _little_endian(dt):
        raise ValueError("attribute field %r is big-endian: little-endian records only" % (name,))
    return int(off), code, ATTR_DTYPE[code]


def resolve_attribute(records, attribute):
    """(offset, type code, numpy dtype) of what a caller passed as `attribute`: a field name of structured records
    (attribute_of), or — the only way for raw (n, point_step) uint8 records — an explicit (offset, type code) pair.  ValueError
    for what attribute_of refuses and for an unknown type code; the offset is the native layers' to judge."""
    if isinstance(attribute, str):
        return attribute_of(np.asarray(records).dtype, attribute)
    try:
        off, code = (int(v) for v in attribute)
    except (TypeError, ValueError):
        raise ValueError("attribute: a field name or an (offset, type code) pair, got %r" % (attribute,)) from None
    if code not in ATTR_DTYPE:
        raise ValueError("attribute: unknown type code %d" % code)
    return off, code, ATTR_DTYPE[code]


def attribute_view(words, dtype):
    """The native layers' uint32 words as the field's dtype: the low bytes of every word, reinterpreted (an INT16 of -1 travels as
    0x0000ffff and comes back as -1; a float32 keeps its bits)."""
    w = np.ascontiguousarray(words, dtype="<u4")
    dt = np.dtype(dtype)
    return w.astype("<u%d" % dt.itemsize).view(dt.newbyteorder("<"))


def check_layout(layout):
    """An explicit layout (six integers) as a RecordLayout; ValueError where the native layers would refuse it."""
    lay = RecordLayout(*(int(v) for v in layout))
    if not POINT_STEP_MIN <= lay.point_step <= POINT_STEP_MAX:
        raise ValueError("point_step %d outside %d .. %d" % (lay.point_step, POINT_STEP_MIN, POINT_STEP_MAX))
    for name in ("off_x", "off_y", "off_z"):
        if not 0 <= getattr(lay, name) <= lay.point_step - 4:
            raise ValueError("%s = %d does not lie inside the record" % (name, getattr(lay, name)))
    if lay.t_type != T_NONE:
        if lay.t_type not in _TIME_WIDTH:
            raise ValueError("unknown t_type %d" % lay.t_type)
        if not 0 <= lay.off_t <= lay.point_step - _TIME_WIDTH[lay.t_type]:
            raise ValueError("off_t = %d does not lie inside the record" % lay.off_t)
    return lay


def resolve(records, time_field=None, layout=None):
    """(n_records, RecordLayout) of what Pipeline.computeRecordsStamped was given: a C-contiguous 1-D structured array (layout
    from its dtype), or an (n, point_step) uint8 array with an explicit `layout`.  The array itself is not copied."""
    if not isinstance(records, np.ndarray):
        raise ValueError("records must be a numpy array")
    if not records.flags["C_CONTIGUOUS"]:
        raise ValueError("records must be C-contiguous")
    if records.dtype.fields is not None:
        if records.ndim != 1:
            raise ValueError("structured records must be 1-D")
        lay = layout_of(records.dtype, time_field) if layout is None else check_layout(layout)
        if lay.point_step != records.dtype.itemsize:
            raise ValueError("layout.point_step differs from the dtype's itemsize")
        return int(records.shape[0]), lay
    if records.dtype != np.uint8 or records.ndim != 2:
        raise ValueError("records must be a 1-D structured array or an (n, point_step) uint8 array")
    if layout is None:
        raise ValueError("raw uint8 records need an explicit layout")
    lay = check_layout(layout)
    if lay.point_step != records.shape[1]:
        raise ValueError("layout.point_step differs from the rows' length")
    return int(records.shape[0]), lay


MAX_SOURCES = 8  # MADICP_MAX_SOURCES
MAX_RECORDS = 2 ** 30


class Source:
    """One sensor's records in a frame of several (madicp_record_source): the buffer as resolve() takes it, the range bounds IN
    THE SENSOR'S FRAME, `attribute` (None, or the field carried as the points' attribute: resolve_attribute), `sensor_to_base` (4x4, None = identity: the upper 3x4 is used as given, orthonormality is the caller's
    business) and the time field's way onto the clock all sources share: common = field * time_scale + time_offset (uint32
    nanoseconds: time_scale=1e-9, time_offset = the message's header stamp RELATIVE TO THE FRAME'S START — an absolute epoch
    as offset eats the nanoseconds)."""

    __slots__ = ("records", "min_range", "max_range", "sensor_to_base", "time_scale", "time_offset", "kitti_correction",
                 "time_field", "layout", "attribute")

    def __init__(self, records, min_range, max_range, sensor_to_base=None, time_scale=1.0, time_offset=0.0, kitti_correction=False,
                 time_field=None, layout=None, attribute=None):
        self.records = records
        self.min_range = min_range
        self.max_range = max_range
        self.sensor_to_base = sensor_to_base
        self.time_scale = time_scale
        self.time_offset = time_offset
        self.kitti_correction = kitti_correction
        self.time_field = time_field
        self.layout = layout
        self.attribute = attribute  # None, a field's name, or (offset, type code): resolve_attribute


ResolvedSource = collections.namedtuple(
    "ResolvedSource", "records n_records layout R t min_range max_range time_scale time_offset kitti_correction attribute")
# (attribute: (offset, type code) — (0, A_NONE) for a source that names none)


def resolve_sources(sources):
    """[ResolvedSource] of what Pipeline.computeSourcesStamped was given — resolve() per source, R (9 floats, row-major) and t (3)
    of sensor_to_base.  ValueError where the native layers would refuse: no source or more than MAX_SOURCES, a source that is not
    a Source, what resolve() refuses, an empty source or more than 2^30 records in all, a sensor_to_base that is not 4x4 or not
    finite in its upper 3x4, a time_scale that is not finite and > 0, a non-finite time_offset, sources with and without a time
    field; what resolve_attribute refuses, sources with and without an attribute, attribute dtypes that differ over the sources."""
    sources = list(sources)
    if not 1 <= len(sources) <= MAX_SOURCES:
        raise ValueError("1 .. %d sources, got %d" % (MAX_SOURCES, len(sources)))
    out = []
    for k, src in enumerate(sources):
        if not isinstance(src, Source):
            raise ValueError("source %d is not a mad_icp_amd.records.Source" % k)
        n, lay = resolve(src.records, src.time_field, src.layout)
        if n < 1:
            raise ValueError("source %d holds no records" % k)
        if src.sensor_to_base is None:
            T = np.eye(4)
        else:
            T = np.asarray(src.sensor_to_base, dtype=np.float64)
            if T.shape != (4, 4):
                raise ValueError("source %d: sensor_to_base must be 4x4" % k)
            if not np.isfinite(T[:3]).all():
                raise ValueError("source %d: sensor_to_base has a non-finite entry" % k)
        scale, offset = float(src.time_scale), float(src.time_offset)
        if not (np.isfinite(scale) and scale > 0.0):
            raise ValueError("source %d: time_scale must be finite and > 0" % k)
        if not np.isfinite(offset):
            raise ValueError("source %d: time_offset must be finite" % k)
        out.append(ResolvedSource(src.records, n, lay, tuple(float(v) for v in T[:3, :3].reshape(-1)),
                                  tuple(float(v) for v in T[:3, 3]), float(src.min_range), float(src.max_range), scale, offset,
                                  bool(src.kitti_correction),
                                  (0, A_NONE) if src.attribute is None else resolve_attribute(src.records, src.attribute)[:2]))
    if sum(r.n_records for r in out) > MAX_RECORDS:
        raise ValueError("more than 2^30 records in all")
    if len({r.layout.t_type != T_NONE for r in out}) != 1:
        raise ValueError("a time field in every source or in none")
    if len({r.attribute[1] != A_NONE for r in out}) != 1:
        raise ValueError("an attribute in every source or in none")
    if len({r.attribute[1] for r in out}) != 1:
        raise ValueError("the same attribute dtype in every source")
    return out
