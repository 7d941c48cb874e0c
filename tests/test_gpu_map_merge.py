"""Context.map_merge_rows (madicp_map_merge_rows: fe::rows_claim, fe::voxel_mark, the tile scan, fe::rows_append, fe::rows_combine)
on the scenarios of tests/test_host_map_merge.py: every column, count and removal-log entry byte-equal to the restatement
(tests/map_merge_ref.py) after every step, and to the host twin driven alike — batch sizes around a wavefront and a scan tile with
growth inside the merge, all entries on one key, duplicates straddling lane 63 / 64 and entry 1023 / 1024, a batch half present,
evidence that saturates, rows frozen, closed and born closed, NaN rows and words, every refusal, a map restored from its own
columns (and from the twin's, and the reverse), and moments that add."""
import ctypes as C

import numpy as np
import pytest

import map_merge_ref as G
import test_host_map_merge as H
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps and twin are fixtures)
from test_host_map_merge import KIND_NAMES, twin  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev(ctx, maps):
    return lambda kind="plain", **k: maps.dev(ctx, **{"voxel": G.VOXEL, **G.KINDS[kind], **k})


def same_seen(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        G.same(x, y)


@pytest.mark.parametrize("n", G.SIZES)
def test_device_merge_is_the_restatement_and_the_twin_at_every_size(dev, twin, n):
    for kind in KIND_NAMES:
        same_seen(H.run_sized(dev, kind, n), H.run_sized(twin, kind, n))


@pytest.mark.parametrize("n", [1025, 4097])
def test_device_merge_of_n_entries_on_one_key(dev, twin, n):
    """every lane claims the same slot, lowers the same owner word and adds to the same evidence word and ten moment words"""
    for kind in KIND_NAMES:
        same_seen(H.run_one_key(dev, kind, n), H.run_one_key(twin, kind, n))


@pytest.mark.parametrize("name", list(H.SCENARIOS))
def test_device_merge_scenarios(dev, twin, name):
    for kind in KIND_NAMES:
        same_seen(H.SCENARIOS[name](dev, kind), H.SCENARIOS[name](twin, kind))


def test_device_merge_evidence_saturates(dev, twin):
    for kind in ("ev", "attr_ev", "ev_mom", "attr_ev_mom"):
        same_seen(H.run_saturating(dev, kind), H.run_saturating(twin, kind))


def test_device_merge_and_the_freeze(dev, twin):
    for kind in ("ev_mom", "attr_ev_mom"):
        same_seen(H.run_freezes(dev, kind), H.run_freezes(twin, kind))


def test_device_merge_refusals_leave_everything(ctx, dev, twin):
    def raw(m, voxel, b, n=None, answers=True, handle=True):
        added, rows = C.c_int64(-7), C.c_int64(-7)
        rc = capi.hip_lib().madicp_map_merge_rows(ctx._h if handle else None, m.mid, float(voxel), *H.raw_args(b, n),
                                                  C.byref(added) if answers else None, C.byref(rows) if answers else None)
        return rc, added.value, rows.value

    for kind in KIND_NAMES:
        G.same(H.run_refusals(dev, kind, raw), H.run_refusals(twin, kind, H.host_raw))
    m = dev("plain")
    b = G.entries({}, G.distinct_keys(3, 1), 2)
    added, rows = C.c_int64(-7), C.c_int64(-7)
    assert capi.hip_lib().madicp_map_merge_rows(ctx._h, 987654, G.VOXEL, *H.raw_args(b), C.byref(added), C.byref(rows)) == G.INVALID  # unknown id
    assert (added.value, rows.value, m.size()) == (-7, -7, 0)


EXACT = ("folds", "clearing", "prune", "log", "query", "score")  # what is integers or stored bits: equal between device and twin


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_device_map_restored_from_its_columns_is_the_map(dev, twin, kind):
    d, h = H.run_round_trip(dev, kind), H.run_round_trip(twin, kind)
    for name in EXACT:
        assert d[name] == h[name], (kind, name)
    G.same(d["columns"], h["columns"])


@pytest.mark.parametrize("kind", ["plain", "attr_ev_mom"])
def test_a_save_crosses_between_device_and_twin(dev, twin, kind):
    """a device map restored from the host twin's columns, and the reverse: the same map either way"""
    import cloud_export_ref as E

    src_h, src_d = twin(kind), dev(kind)
    for i in range(2):
        cloud, words = E.gaussian(1500, 70 + i, scale=2.0), np.arange(1500, dtype=np.uint32) * 3 + i
        assert src_h.insert(cloud, *E.IDENTITY, words) == src_d.insert(cloud, *E.IDENTITY, words)
    saved_h, saved_d = G.columns(src_h), G.columns(src_d)
    G.same(saved_h, saved_d)
    to_d, to_h = dev(kind, initial_rows=1), twin(kind, initial_rows=1)
    assert G.call(to_d, saved_h) == G.call(to_h, saved_d) == (src_h.size(), src_h.size())
    G.same(G.columns(to_d), saved_h)
    G.same(G.columns(to_h), saved_d)
    more = E.gaussian(1200, 80, scale=2.5)
    assert to_d.insert(more, *E.IDENTITY, None) == to_h.insert(more, *E.IDENTITY, None) == src_d.insert(more, *E.IDENTITY, None)
    G.same(G.columns(to_d), G.columns(to_h))
    G.same(G.columns(to_d), G.columns(src_d))


def test_device_moments_of_two_maps_add(dev, twin):
    G.same(H.run_additivity(dev), H.run_additivity(twin))
