"""mad_icp_amd.records.Source / resolve_sources — what Pipeline.computeSourcesStamped reads a rig's buffers by — and what they
refuse with a ValueError before any native layer is asked.  No GPU, no native library."""
import numpy as np
import pytest

from mad_icp_amd import records
from mad_icp_amd.records import Source, resolve_sources

DT22 = np.dtype(dict(names=["x", "y", "z", "t"], formats=["<f4", "<f4", "<f4", "<u4"], offsets=[0, 4, 8, 18], itemsize=22))
DT16 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("time", "<f4")])
DT12 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])


def test_defaults_and_resolution():
    a, b = np.zeros(5, DT22), np.zeros(7, DT16)
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.5, -0.25, 1.0]
    r = resolve_sources([Source(a, 0.7, 120.0), Source(b, 1.0, 50.0, sensor_to_base=T, time_scale=2.0, time_offset=-0.5, kitti_correction=True)])
    assert len(r) == 2
    assert r[0].records is a and r[0].n_records == 5 and r[0].layout == records.RecordLayout(22, 0, 4, 8, 18, records.T_U32)
    assert r[0].R == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0) and r[0].t == (0.0, 0.0, 0.0)
    assert (r[0].min_range, r[0].max_range, r[0].time_scale, r[0].time_offset, r[0].kitti_correction) == (0.7, 120.0, 1.0, 0.0, False)
    assert r[1].records is b and r[1].n_records == 7 and r[1].layout == records.RecordLayout(16, 0, 4, 8, 12, records.T_F32)
    assert r[1].R == (0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0) and r[1].t == (0.5, -0.25, 1.0)       # row-major
    assert (r[1].min_range, r[1].max_range, r[1].time_scale, r[1].time_offset, r[1].kitti_correction) == (1.0, 50.0, 2.0, -0.5, True)


def test_time_field_and_explicit_layout_per_source():
    a, b = np.zeros(5, DT22), np.zeros((7, 22), np.uint8)
    r = resolve_sources([Source(a, 0.7, 120.0, time_field=False), Source(b, 0.7, 120.0, layout=(22, 0, 4, 8, 0, records.T_NONE))])
    assert [x.layout.t_type for x in r] == [records.T_NONE, records.T_NONE]
    r = resolve_sources([Source(a, 0.7, 120.0, time_field="t"), Source(b, 0.7, 120.0, layout=(22, 0, 4, 8, 18, records.T_F32))])
    assert [x.layout.t_type for x in r] == [records.T_U32, records.T_F32]
    assert len(resolve_sources([Source(a, 0.7, 120.0)] * records.MAX_SOURCES)) == 8
    assert len(resolve_sources(iter([Source(a, 0.7, 120.0)]))) == 1                                    # any iterable


def test_refusals():
    a = np.zeros(5, DT22)
    ok = Source(a, 0.7, 120.0)
    bad_T = np.eye(4)
    bad_T[1, 3] = np.nan
    inf_T = np.eye(4)
    inf_T[2, 2] = np.inf
    refused = [
        [],                                                              # no source
        [ok] * 9,                                                        # more than eight
        [ok, (a, 0.7, 120.0)],                                           # not a Source
        [ok, Source(a[:0], 0.7, 120.0)],                                 # an empty source
        [ok, Source(a[::2], 0.7, 120.0)],                                # what resolve() refuses: not contiguous
        [ok, Source(np.zeros((5, 22), np.uint8), 0.7, 120.0)],           # ... raw bytes without a layout
        [ok, Source(a, 0.7, 120.0, layout=(22, 0, 4, 8, 19, records.T_U32))],  # ... a field outside the record
        [Source(a, 0.7, 120.0, sensor_to_base=np.eye(3))],               # not 4x4
        [Source(a, 0.7, 120.0, sensor_to_base=bad_T)],
        [Source(a, 0.7, 120.0, sensor_to_base=inf_T)],
        [Source(a, 0.7, 120.0, time_scale=0.0)],
        [Source(a, 0.7, 120.0, time_scale=-1.0)],
        [Source(a, 0.7, 120.0, time_scale=np.nan)],
        [Source(a, 0.7, 120.0, time_scale=np.inf)],
        [Source(a, 0.7, 120.0, time_offset=np.nan)],
        [Source(a, 0.7, 120.0, time_offset=-np.inf)],
        [ok, Source(np.zeros(5, DT12), 0.7, 120.0)],                     # with and without a time field
        [Source(a, 0.7, 120.0, time_field=False), ok],
    ]
    for sources in refused:
        with pytest.raises(ValueError):
            resolve_sources(sources)
    bottom = np.eye(4)
    bottom[3] = [np.nan, 7.0, 7.0, 7.0]                                 # (the last row of sensor_to_base is not read)
    assert resolve_sources([Source(a, 0.7, 120.0, sensor_to_base=bottom)])[0].R[0] == 1.0


def test_total_record_count_is_bounded(monkeypatch):
    a = np.zeros(5, DT22)
    monkeypatch.setattr(records, "MAX_RECORDS", 9)
    assert len(resolve_sources([Source(a, 0.7, 120.0)])) == 1
    with pytest.raises(ValueError):
        resolve_sources([Source(a, 0.7, 120.0), Source(a, 0.7, 120.0)])
