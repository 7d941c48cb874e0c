"""The per-point attribute through Pipeline — computeRecordsStamped(..., attribute=) / Source(..., attribute=), registeredScan(...,
with_attribute=True), setMapAccumulation(..., with_attribute=True) / mapCloud(..., with_attribute=True) — on the 8-frame 16 x 450
drive of tests/test_gpu_pipeline_registered_scan.py, both front-ends.  The attribute is the RECORD INDEX (a uint32 written into
idle bytes of every record at an odd offset), so row j of the retained scan must be the deskew of record attr[j]; the poses are
those of the same drive without the attribute, bit for bit; the map's column is the restatement of tests/attribute_ref.py folded
over the frames.  Everything is exact equality."""
import copy

import numpy as np
import pytest

import attribute_ref as A
import cloud_export_ref as E
from mad_icp_amd import capi
from mad_icp_amd.records import A_UINT32, Source
from test_gpu_pipeline_map import built_from
from test_gpu_pipeline_registered_scan import HI, HZ, LAY, LO, bits, drive, pipeline  # noqa: F401  (drive: the module-scoped fixture)

pytestmark = pytest.mark.gpu

VOXEL = 0.5
IDX_OFF = {22: 13, 48: 29}  # idle bytes of the two layouts of the drive, odd: a uint32 there straddles two dwords
DT22 = np.dtype({"names": ["x", "y", "z", "idx", "t"], "formats": ["<f4", "<f4", "<f4", "<u4", "<u4"], "offsets": [0, 4, 8, 13, 18], "itemsize": 22})


def indexed(raw, first):
    """a copy of (n, step) uint8 records with the uint32 `first + record number` at IDX_OFF[step]"""
    out = np.array(raw, copy=True)
    n, step = out.shape
    out[:, IDX_OFF[step]:IDX_OFF[step] + 4] = (np.arange(n, dtype="<u4") + np.uint32(first)).view(np.uint8).reshape(n, 4)
    return out


def with_index(f):
    """the frame's records with the index field: (structured one-head records, its survivors' indices, two-head sources, theirs)"""
    raw = indexed(f["records"].view(np.uint8).reshape(-1, LAY.point_step), 0)
    kept = np.nonzero(A.keep_mask(Source(raw, LO, HI, layout=LAY)))[0].astype(np.uint32)
    sources, s_kept, first = [], [], 0
    for src in f["sources"]:
        s = copy.copy(src)
        s.records = indexed(src.records, first)
        s.attribute = (IDX_OFF[s.records.shape[1]], A_UINT32)
        s_kept.append(np.nonzero(A.keep_mask(s))[0].astype(np.uint32) + np.uint32(first))
        first += s.records.shape[0]
        sources.append(s)
    return raw.reshape(-1).view(DT22), kept, sources, np.concatenate(s_kept)


def feed(p, kind, i, rec, sources, attribute=True, time_field=None):
    if kind == "records":
        p.computeRecordsStamped(0.1 * i, rec, LO, HI, time_field=time_field, attribute="idx" if attribute else None)
    else:
        p.computeSourcesStamped(0.1 * i, sources if attribute else [_plain(s) for s in sources])


def _plain(src):
    s = copy.copy(src)
    s.attribute = None
    return s


@pytest.mark.parametrize("kind,device_frontend", [("records", True), ("records", False), ("sources", True), ("sources", False)])
def test_stamped_drive(natives, drive, kind, device_frontend):
    on, off = pipeline(True, device_frontend, keep=True), pipeline(True, device_frontend)
    on.setMapAccumulation(VOXEL, with_attribute=True)
    assert on.mapWithAttribute() and not off.mapWithAttribute()
    ref = A.AttrMap(VOXEL)
    for i, f in enumerate(drive):
        rec, kept, sources, s_kept = with_index(f)
        want = s_kept if kind == "sources" else kept
        feed(on, kind, i, rec, sources)
        feed(off, kind, i, rec, sources, attribute=False)
        assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(off.currentPose()))), i
        assert on.keyframeID() == off.keyframeID() and on.isMapUpdated() == off.isMapUpdated(), i
        T = np.asarray(on.currentPose())
        cloud = built_from(kind, f, i, np.asarray(on.trajectory()))
        # the retained scan: stamped deskews keep the input order, so row j is the deskew of survivor j — record attr[j]
        rows, attr = on.registeredScan(0.0, "sensor", with_attribute=True)
        assert attr.dtype == np.dtype("<u4") and np.array_equal(attr, want), i
        assert E.same_bits(rows, E.export_f32(cloud, *E.IDENTITY, 0.0)) and rows.tobytes() == on.registeredScan(0.0, "sensor").tobytes()
        for frame, X in (("map", (T[:3, :3], T[:3, 3])), ("sensor", E.IDENTITY)):
            rows, attr = on.registeredScan(VOXEL, frame, with_attribute=True)
            want_rows, want_attr = A.export(cloud, want, X[0], X[1], VOXEL)
            assert E.same_bits(rows, want_rows) and np.array_equal(attr, want_attr), (i, frame)
            assert rows.tobytes() == on.registeredScan(VOXEL, frame).tobytes() and rows.shape[0] < cloud.shape[0]
        # the map
        before = ref.size
        assert ref.insert(cloud, want, T[:3, :3], T[:3, 3]) > 0
        rows, attr = on.mapCloud(0, with_attribute=True)
        assert E.same_bits(rows, ref.rows()) and attr.dtype == np.dtype("<u4") and np.array_equal(attr, ref.attr()), i
        rows, attr = on.mapCloud(before, with_attribute=True)
        assert E.same_bits(rows, ref.rows(before)) and np.array_equal(attr, ref.attr(before))
    assert np.array_equal(bits(np.asarray(on.trajectory())), bits(np.asarray(off.trajectory())))
    assert not np.array_equal(np.asarray(on.trajectory())[-1], np.eye(4))


@pytest.mark.parametrize("device_frontend", [True, False])
def test_azimuth_deskew_end_to_end(natives, ctx, drive, device_frontend):
    """records WITHOUT a time field and deskew = true: from the third frame on the azimuth deskew re-orders the points, and the
    column with them.  Host front-end: against madicp_host_debug_deskew (the same code: the rows; at zero motion it only sorts: the
    order).  Device front-end: against the C ABI on a context of its own — upload, set_attr, madicp_cloud_deskew, export."""
    on, off = pipeline(True, device_frontend, keep=True), pipeline(True, device_frontend)
    permuted = 0
    for i, f in enumerate(drive[:5]):
        rec, kept, sources, _ = with_index(f)
        feed(on, "records", i, rec, sources, time_field=False)
        feed(off, "records", i, rec, sources, attribute=False, time_field=False)
        assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(off.currentPose()))), i
        rows, attr = on.registeredScan(0.0, "sensor", with_attribute=True)
        pts = f["pts"]
        assert rows.shape == (pts.shape[0], 3) and sorted(attr.tolist()) == kept.tolist()
        if i < 2:  # (no deskew is due yet)
            assert np.array_equal(attr, kept) and np.array_equal(rows, pts.astype(np.float32))
            continue
        traj = np.asarray(on.trajectory())
        pos = np.full(rec.shape[0], -1, np.int64)
        pos[kept] = np.arange(kept.shape[0])
        permuted += int(not np.array_equal(attr, kept))
        if device_frontend:
            _, vel, _ = capi.host_deskew(pts, traj[i - 2], traj[i - 1], HZ)
            cid = ctx.cloud_upload(pts)
            try:
                ctx.cloud_set_attr(cid, kept)
                ctx.cloud_deskew(cid, vel, HZ)
                want_rows, want_attr = ctx.cloud_export_f32_attr(cid, *E.IDENTITY, 0.0)
            finally:
                ctx.cloud_release(cid)
            assert rows.tobytes() == want_rows.tobytes() and np.array_equal(attr, want_attr), i
        else:
            moved, _, _ = capi.host_deskew(pts, traj[i - 2], traj[i - 1], HZ)
            only_sorted, _, _ = capi.host_deskew(pts, np.eye(4), np.eye(4), HZ)
            assert E.same_bits(rows, E.export_f32(moved, *E.IDENTITY, 0.0)), i
            assert np.array_equal(pts[pos[attr]], only_sorted), i  # row j is record attr[j]
    assert permuted == 3


def test_frames_without_an_attribute(natives, drive):
    """a frame fed without an attribute: its retained scan carries none (registeredScan(with_attribute=True) says so) and its map
    rows get the word 0; a map made without the column refuses mapCloud(with_attribute=True)"""
    p, plain = pipeline(True, True, keep=True), pipeline(True, True)
    p.setMapAccumulation(VOXEL, with_attribute=True)
    plain.setMapAccumulation(VOXEL)
    ref = A.AttrMap(VOXEL)
    for i, f in enumerate(drive[:3]):
        rec, kept, sources, _ = with_index(f)
        feed(p, "records", i, rec, sources, attribute=(i != 1))
        feed(plain, "records", i, rec, sources, attribute=False)
        T = np.asarray(p.currentPose())
        cloud = built_from("records", f, i, np.asarray(p.trajectory()))
        ref.insert(cloud, kept if i != 1 else None, T[:3, :3], T[:3, 3])
        if i == 1:
            with pytest.raises(RuntimeError, match="no attribute"):
                p.registeredScan(0.0, "sensor", with_attribute=True)
            assert p.registeredScan(0.0, "sensor").shape == (cloud.shape[0], 3)
        else:
            assert np.array_equal(p.registeredScan(0.0, "sensor", with_attribute=True)[1], kept)
        rows, attr = p.mapCloud(0, with_attribute=True)
        assert E.same_bits(rows, ref.rows()) and np.array_equal(attr, ref.attr()), i
        assert rows.tobytes() == plain.mapCloud().tobytes()
    assert (ref.attr() == 0).sum() >= ref.words[1].shape[0] > 0
    with pytest.raises(RuntimeError, match="without the attribute"):
        plain.mapCloud(0, with_attribute=True)


def test_refusals(natives, drive):
    rec, kept, sources, _ = with_index(drive[0])
    p = pipeline(True, True, keep=True)
    with pytest.raises(ValueError):
        p.computeRecordsStamped(0.0, rec, LO, HI, attribute="intensity")  # no such field
    with pytest.raises(ValueError):
        p.computeRecordsStamped(0.0, rec.view(np.uint8).reshape(-1, 22), LO, HI, layout=tuple(LAY), attribute=(19, A_UINT32))  # past the end
    mixed = [sources[0], _plain(sources[1])]
    with pytest.raises(ValueError):
        p.computeSourcesStamped(0.0, mixed)
    other = copy.copy(sources[1])
    other.attribute = (IDX_OFF[48], 4)
    with pytest.raises(ValueError):
        p.computeSourcesStamped(0.0, [sources[0], other])
    p.computeRecordsStamped(0.0, rec.view(np.uint8).reshape(-1, 22), LO, HI, layout=tuple(LAY), attribute=(IDX_OFF[22], A_UINT32))
    assert np.array_equal(p.registeredScan(0.0, "sensor", with_attribute=True)[1], kept)
