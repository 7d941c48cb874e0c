"""The layout of a driver's point records, read off a numpy dtype.

A LiDAR driver delivers a PointCloud2-style byte buffer: records `point_step` bytes apart, float32 x / y / z at byte offsets and
— usually — a per-point time field named `t`, `timestamp` or `time` (uint32 nanoseconds, float32 or float64 seconds).  A reader
such as the reference's apps/utils/point_cloud2.py::read_points returns it as a 1-D numpy STRUCTURED array; this module turns
that array's dtype into the six integers of madicp_record_layout (include/madicp_hip.h), which is all the native layers take:

    layout_of(dtype, time_field=None) -> RecordLayout(point_step, off_x, off_y, off_z, off_t, t_type)
    resolve(records, time_field=None, layout=None) -> (n_records, RecordLayout)     what Pipeline.computeRecordsStamped calls

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
