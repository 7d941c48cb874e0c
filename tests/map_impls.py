"""The voxel map behind the interface the restatements' replays drive (tests/*_ref.py: insert / prune / clear_rays / query, the
columns, the removal log), once for the host twin (capi.HostMap) and once for the device map (capi.DeviceMap), and the fixture
that closes what a test made.  What is here is test plumbing only: on the device a scan is uploaded, given its words, used and
released; where two suites do that differently the adapter takes a flag and the suite passes it."""
import contextlib
import types

import numpy as np
import pytest

from mad_icp_amd import capi


def refusable(call, *a):
    """the answer of a capi call, None where it is refused for capacity (error -4)"""
    try:
        return call(*a)
    except capi.MadIcpError as e:
        if "error -4" not in str(e):
            raise
        return None


class MapImpl:
    """what does not depend on where the map lives.  tracking: the removal log from the start; refusals: a fold or removal
    refused for capacity answers None (tests/map_removed_ref.py's replays expect those)."""

    def __init__(self, map_, with_attr, evidence, max_count, tracking, refusals):
        self.map, self.with_attr, self.params, self.max_count, self.refusals = map_, with_attr, evidence, max_count, refusals
        if tracking:
            self.track(True)

    def _answer(self, call, *a):
        return refusable(call, *a) if self.refusals else call(*a)

    def prune(self, c, r, wm=0):
        return self._answer(self.map.prune, c, r, wm)

    def size(self):
        return self.map.size()

    def rows(self, first_row=0):
        return self.map.download_f32(first_row)

    def keys(self):
        return self.map.download_keys()

    def words(self):
        return self.map.download_attr() if self.with_attr else None

    def evidence(self):
        return self.map.download_evidence() if self.params is not None else None

    def confirmed(self, min_e):
        return self.map.download_min_evidence(min_e, with_keys=True, with_attr=self.with_attr, with_ev=True)

    def moments(self):
        return self.map.download_moments() if self.max_count is not None else None

    def surfels(self, first_row=0):
        return self.map.download_surfels(first_row)

    def columns(self):
        """every column the map has, by name (the rows, keys and words behind one download_rows)"""
        got = dict(zip(("xyz", "keys", "attr"), self.map.download_rows(with_keys=True, with_attr=self.with_attr)))
        if self.params is not None:
            got["evidence"] = self.map.download_evidence()
        if self.max_count is not None:
            got["moments"] = self.map.download_moments()
        return got

    def removed_count(self):
        return self.map.removed_count()

    def take(self):
        return self.map.take_removed(self.with_attr)

    def track(self, on):
        self.map.track_removed(on)

    def clear(self):
        self.map.clear()

    reset = wipe = clear

    def close(self):
        self.map.close()


class HostImpl(MapImpl):
    """insert_attr: whether a fold goes through madicp_host_map_insert_attr (default: on a map with the attribute column)"""

    def __init__(self, voxel, initial_rows=64, max_rows=1 << 24, with_attr=False, evidence=None, max_count=None, tracking=False,
                 refusals=False, insert_attr=None):
        self.insert_attr = with_attr if insert_attr is None else insert_attr
        super().__init__(capi.HostMap.create(voxel, initial_rows, max_rows, with_attr, evidence, max_count), with_attr, evidence, max_count,
                         tracking, refusals)

    @property
    def h(self):
        return self.map._h

    def insert(self, pts, R, t, words=None, key=None):
        return self._answer(self.map.insert, pts, R, t, *((words,) if self.insert_attr else ()))

    def clear_rays(self, pts, R, t, origin=(0.0, 0.0, 0.0), margin=0.0, wm=0, words=None, key=None):
        return self._answer(self.map.clear_rays, pts, R, t, origin, margin, wm)

    def query(self, cloud, R, t, reach, max_dist, per_point=True, with_keys=False, with_attr=False, with_ev=False):
        return self.map.query(cloud, R, t, reach, max_dist, per_point, with_keys, with_attr, with_ev)

    def register(self, cloud, R, t, iterations, **kw):
        return self.map.register(cloud, R, t, iterations, **kw)


class DevImpl(MapImpl):
    """set_attr: whether a scan that comes with words gets them as its attribute column (default: for a map with the column).
    A scan given with a `key` stays resident under it until close() and is used again, as it is, wherever the key comes back."""

    def __init__(self, ctx, voxel, initial_rows=64, max_rows=1 << 24, with_attr=False, evidence=None, max_count=None, tracking=False,
                 refusals=False, set_attr=None):
        self.ctx, self.clouds = ctx, {}
        self.set_attr = with_attr if set_attr is None else set_attr
        super().__init__(capi.DeviceMap.create(ctx, voxel, initial_rows, max_rows, with_attr, evidence, max_count), with_attr, evidence,
                         max_count, tracking, refusals)

    @property
    def mid(self):
        return self.map.mid

    def cloud(self, pts, words=None):
        """the id of pts as a resident cloud, the caller's to release"""
        cid = self.ctx.cloud_upload(np.ascontiguousarray(pts, np.float64).reshape(-1, 3))
        try:
            if words is not None and self.set_attr:
                self.ctx.cloud_set_attr(cid, words)
        except BaseException:
            self.ctx.cloud_release(cid)
            raise
        return cid

    @contextlib.contextmanager
    def resident(self, pts, words=None, key=None):
        if key is not None:
            if key not in self.clouds:
                self.clouds[key] = self.cloud(pts, words)
            yield self.clouds[key]
            return
        cid = self.cloud(pts, words)
        try:
            yield cid
        finally:
            self.ctx.cloud_release(cid)

    def insert(self, pts, R, t, words=None, key=None):
        with self.resident(pts, words, key) as cid:
            return self._answer(self.map.insert, cid, R, t)

    def clear_rays(self, pts, R, t, origin=(0.0, 0.0, 0.0), margin=0.0, wm=0, words=None, key=None):
        with self.resident(pts, words, key) as cid:
            return self._answer(self.map.clear_rays, cid, R, t, origin, margin, wm)

    def query(self, cloud, R, t, reach, max_dist, per_point=True, with_keys=False, with_attr=False, with_ev=False):
        with self.resident(cloud) as cid:
            return self.map.query(cid, R, t, reach, max_dist, per_point, with_keys, with_attr, with_ev)

    def register(self, cloud, R, t, iterations, **kw):
        with self.resident(cloud) as cid:
            return self.map.register(cid, R, t, iterations, **kw)

    def close(self):
        for cid in self.clouds.values():
            self.ctx.cloud_release(cid)
        self.map.close()


@pytest.fixture
def maps(natives):
    """maps.host(...) makes a HostImpl and maps.dev(ctx, ...) a DevImpl; all of them are closed at the end of the test"""
    made = []

    def make(cls):
        def new(*a, **k):
            made.append(cls(*a, **k))
            return made[-1]

        return new

    yield types.SimpleNamespace(host=make(HostImpl), dev=make(DevImpl))
    for m in made:
        m.close()
