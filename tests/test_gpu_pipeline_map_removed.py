"""Pipeline.setMapTrackRemoved / mapRemovedRows / mapNewRows(with_keys=True) / mapKeys — a map that a consumer can mirror — on the
8-frame 16 x 450 drive of tests/test_gpu_pipeline_registered_scan.py with free-space clearing and a range, both front-ends: a
mad_icp_amd.map_mirror.MapMirror polled every frame, every third frame and only once at the end equals the map at every poll; what
each poll takes is the restatement's of tests/map_removed_ref.py (RefDrive), bit for bit; a Pipeline that does not track has the
same poses, map bytes, mapRemoved() and mapNewRows() stream; clearMap empties the log; a full log skips removals and says so; the
front-end switched mid-drive.  Everything is exact equality."""
import numpy as np
import pytest

import cloud_export_ref as E
import map_removed_ref as Rm
from mad_icp_amd.map_mirror import MapMirror
from test_gpu_pipeline_map import built_from
from test_gpu_pipeline_registered_scan import bits, drive, feed, pipeline  # noqa: F401  (drive: the module-scoped fixture)

pytestmark = pytest.mark.gpu

VOXEL = 0.5
RADIUS = 8.0  # the drive advances 1 m per frame: a prune every second frame
MARGIN = 0.25
ORIGIN = np.array([0.0, 0.0, 0.125])
BY_HAND = 6  # behind this frame one mapClearRays by hand, with the frame's scan half as far again: it looks through what it folded
CADENCES = {"every": lambda i, last: True, "third": lambda i, last: i % 3 == 2 or last, "end": lambda i, last: last}


class Tap:
    """the Pipeline as MapMirror.update sees it, keeping what the two calls returned"""

    def __init__(self, p):
        self.p, self.gone, self.new = p, None, None

    def mapRemovedRows(self, with_attribute=False):
        self.gone = self.p.mapRemovedRows(with_attribute=with_attribute)
        return self.gone

    def mapNewRows(self, with_attribute=False, with_keys=False):
        self.new = self.p.mapNewRows(with_attribute=with_attribute, with_keys=with_keys)
        return self.new


def tracked(deskew, device_frontend, with_attr, tracking=True):
    p = pipeline(deskew, device_frontend)
    p.setMapAccumulation(VOXEL, with_attribute=with_attr)
    p.setMapClearing(True, MARGIN, ORIGIN)
    p.setMapRange(RADIUS)
    if tracking:
        p.setMapTrackRemoved(True)
    return p


def sorted_map(p, with_attr):
    keys = p.mapKeys()
    order = np.argsort(keys, kind="stable")
    assert np.unique(keys).shape[0] == keys.shape[0]  # the stored key is unique among the rows the map holds
    if with_attr:
        rows, attr = p.mapCloud(0, with_attribute=True)
        return keys[order], rows[order], np.asarray(attr)[order]
    return keys[order], p.mapCloud()[order], None


def holds_the_map(mirror, p, with_attr, at):
    keys, rows, attr = sorted_map(p, with_attr)
    assert mirror.keys().tobytes() == keys.tobytes(), at
    assert E.same_bits(mirror.rows(), rows), at
    if with_attr:
        assert mirror.attr().tobytes() == attr.tobytes(), at


class Consumer:
    """one polling cadence: its Pipeline, its mirror, the restatement with the same cursor, and what it has seen"""

    def __init__(self, cadence, p, with_attr):
        self.cadence, self.p, self.with_attr = cadence, p, with_attr
        self.tap, self.mirror = Tap(p), MapMirror(with_attr)
        self.ref = Rm.RefDrive(VOXEL, RADIUS, margin=MARGIN, origin=ORIGIN)
        self.logged, self.gone_keys, self.back = 0, set(), set()

    def poll(self, at):
        want_k, want_x, want_w = self.ref.removed_rows()
        new_x, new_w, new_k = self.ref.new_rows_keyed()
        assert self.p.mapRemovedRowCount() == want_k.shape[0], at
        removed, added = self.mirror.update(self.tap)
        assert (removed, added) == (want_k.shape[0], new_k.shape[0]), at
        gone, new = self.tap.gone, self.tap.new
        assert gone[0].dtype == np.uint64 and gone[0].tobytes() == want_k.tobytes() and E.same_bits(gone[1], want_x), at
        assert new[-1].dtype == np.uint64 and new[-1].tobytes() == new_k.tobytes() and E.same_bits(new[0], new_x), at
        if self.with_attr:
            assert np.asarray(gone[2]).tobytes() == want_w.tobytes() and np.asarray(new[1]).tobytes() == new_w.tobytes(), at
        assert np.unique(gone[0]).shape[0] == gone[0].shape[0], at  # within one poll the removed keys are distinct
        assert self.p.mapRemovedRowCount() == 0 and self.p.mapNewRows().shape == (0, 3) and not self.p.mapRemovedLogFull(), at
        self.logged += removed
        self.gone_keys.update(gone[0].tolist())
        self.back.update(self.gone_keys.intersection(new[-1].tolist()))  # (removals first: a key of this very poll counts)
        holds_the_map(self.mirror, self.p, self.with_attr, at)


@pytest.mark.parametrize("kind,device_frontend,with_attr,switch_at", [("cloud", True, True, None), ("cloud", False, True, None),
                                                                      ("stamped", True, False, None), ("stamped", False, False, None),
                                                                      ("cloud", True, False, 3), ("cloud", False, True, 3)])
def test_a_mirror_holds_the_map_at_every_poll(natives, drive, kind, device_frontend, with_attr, switch_at):
    deskew = kind != "cloud"
    consumers = [Consumer(c, tracked(deskew, device_frontend, with_attr), with_attr) for c in CADENCES]
    off = tracked(deskew, device_frontend, with_attr, tracking=False)
    lead = consumers[0].p
    assert lead.mapTrackRemoved() and not off.mapTrackRemoved() and lead.mapRemovedRowCount() == 0
    for i, f in enumerate(drive):
        last = i == len(drive) - 1
        for p in [c.p for c in consumers] + [off]:
            if i == switch_at:  # the map, and the log with it, stay where the first fold put them
                p.setDeviceFrontEnd(not device_frontend)
            feed(p, kind, i, f)
            assert np.array_equal(bits(np.asarray(lead.currentPose())), bits(np.asarray(p.currentPose()))), i
        T = np.asarray(lead.currentPose())
        cloud = built_from(kind, f, i, np.asarray(lead.trajectory())) if deskew else f["pts"]
        for c in consumers:
            assert c.ref.frame(cloud, T) is not None
        if i == BY_HAND:
            for c in consumers:
                assert c.p.mapClearRays(cloud * 1.5, T, ORIGIN, MARGIN) == c.ref.clear_rays(cloud * 1.5, T, ORIGIN, MARGIN) > 100
            off.mapClearRays(cloud * 1.5, T, ORIGIN, MARGIN)
        every = consumers[0]
        for c in consumers:
            assert c.p.mapSize() == c.ref.map.size and c.p.mapRemoved() == c.ref.removed and not c.p.mapOverflowed(), (i, c.cadence)
            assert c.p.mapRemovedRowCount() == c.ref.map.removed_count, (i, c.cadence)
            if CADENCES[c.cadence](i, last):
                c.poll((i, c.cadence))
        # not tracking: the same map bytes and the same count of removals — and, polled like the consumer that looks every frame,
        # the same stream of new rows
        assert off.mapRemoved() == lead.mapRemoved() and off.mapCloud().tobytes() == lead.mapCloud().tobytes(), i
        assert off.mapKeys().tobytes() == lead.mapKeys().tobytes() and off.mapRemovedRowCount() == 0, i
        got = off.mapNewRows(with_attribute=True) if with_attr else off.mapNewRows()
        assert (got[0] if with_attr else got).tobytes() == every.tap.new[0].tobytes(), i
    for c in consumers:
        if c.cadence == "end":  # nothing was delivered before the one poll: nothing that left had to be reported
            assert c.logged == 0 and len(c.mirror) == c.p.mapSize() > 0
            continue
        # the log was not empty, and some voxel left the map and came back while the consumer was looking
        assert c.logged > 0 and len(c.back) > 0, (c.cadence, c.logged, len(c.back))
        assert c.ref.cleared > 500 and c.ref.prunes >= 3, c.cadence
    assert np.array_equal(bits(np.asarray(lead.trajectory())), bits(np.asarray(off.trajectory())))
    with pytest.raises(RuntimeError):
        off.mapRemovedRows()  # tracking is off


@pytest.mark.parametrize("device_frontend", [True, False])
def test_clear_map_empties_the_log_and_errors(natives, drive, device_frontend):
    p = pipeline(False, device_frontend)
    for call in (lambda: p.setMapTrackRemoved(True), p.mapRemovedRowCount, p.mapRemovedRows, p.mapKeys):
        with pytest.raises(RuntimeError):
            call()  # accumulation is off
    p = tracked(False, device_frontend, False)
    assert p.mapKeys().shape == (0,) and p.mapRemovedRows()[0].shape == (0,) and p.mapRemovedRows()[1].shape == (0, 3)
    with pytest.raises(RuntimeError):
        p.mapRemovedRows(with_attribute=True)  # the map has no column
    with pytest.raises(RuntimeError):
        p.mapNewRows(with_attribute=True, with_keys=True)
    mirror = MapMirror()
    for i, f in enumerate(drive[:4]):
        feed(p, "cloud", i, f)
        rows, keys = p.mapNewRows(with_keys=True)  # delivered, so that what leaves is logged — and never taken
        assert rows.shape[0] == keys.shape[0]
    with pytest.raises(ValueError):
        p.mapKeys(p.mapSize() + 1)
    assert p.mapKeys(p.mapSize() - 1).tobytes() == p.mapKeys()[-1:].tobytes()
    assert p.mapRemovedRowCount() > 0 and p.mapRemoved() >= p.mapRemovedRowCount()
    p.clearMap()
    assert p.mapRemovedRowCount() == 0 and p.mapSize() == 0 and p.mapTrackRemoved()
    for i in (4, 5, 6):
        feed(p, "cloud", i, drive[i])
        mirror.update(p)
        holds_the_map(mirror, p, False, i)
    assert len(mirror) == p.mapSize() > 0
    p.setMapTrackRemoved(False)  # frees the log
    assert p.mapRemovedRowCount() == 0 and not p.mapTrackRemoved()


@pytest.mark.parametrize("device_frontend", [True, False])
def test_a_full_log_skips_removals_and_says_so(natives, drive, device_frontend):
    """max_points bounds the log: rows are delivered and pruned out, never taken, until the log holds max_points entries — the next
    prune and the next frame's clearing are skipped, map and mirror stay consistent, and a take puts things right"""
    max_points, far = 7500, np.array([1.0e5, 0.0, 0.0])
    assert all(f["pts"].shape[0] <= max_points for f in drive)
    p = pipeline(False, device_frontend)
    p.setMapAccumulation(0.1, False, max_points)
    p.setMapTrackRemoved(True)
    delivered, full_at = [], None  # (every prune empties the map, in row order: the log is the rows delivered, in that order)
    for i, f in enumerate(drive[:-1]):
        feed(p, "cloud", i, f)
        rows, keys = p.mapNewRows(with_keys=True)
        delivered.append((keys, rows))
        assert not p.mapOverflowed() and not p.mapRemovedLogFull() and p.mapPrune(far, 1.0) == rows.shape[0] > 0
        if p.mapRemovedRowCount() >= max_points:
            full_at = i
            break
    assert full_at is not None, "the drive never filled the log"
    n, removed = p.mapRemovedRowCount(), p.mapRemoved()
    p.setMapClearing(True, MARGIN, ORIGIN)
    feed(p, "cloud", full_at + 1, drive[full_at + 1])  # the fold is fine (the map was empty), its clearing is skipped
    assert p.mapRemovedLogFull() and p.mapRemoved() == removed and p.mapRemovedRowCount() == n and not p.mapOverflowed()
    rows, keys = p.mapNewRows(with_keys=True)
    size = p.mapSize()
    assert size == rows.shape[0] > 0 and p.mapPrune(far, 1.0) == 0 and p.mapSize() == size  # the prune by hand is skipped too
    assert p.mapClearRays(drive[full_at + 1]["pts"] * 1.5, np.asarray(p.currentPose()), ORIGIN, MARGIN) == 0 and p.mapSize() == size
    gone_keys, gone_rows = p.mapRemovedRows()
    assert gone_keys.shape[0] == n and not p.mapRemovedLogFull() and p.mapRemovedRowCount() == 0
    assert gone_keys.tobytes() == np.concatenate([k for k, _ in delivered]).tobytes()
    assert gone_rows.tobytes() == np.concatenate([r for _, r in delivered]).tobytes()
    assert p.mapKeys().tobytes() == keys.tobytes() and p.mapCloud().tobytes() == rows.tobytes()  # the skipped removals left the map alone
    assert p.mapPrune(far, 1.0) == size and p.mapRemovedRowCount() == size
