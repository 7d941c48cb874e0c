"""tests/deskew_ref.py (the literal walk of pipeline.cpp:108-119) held to the oracle's Pipeline::deskew and to the host deskew,
on the CPU, for every cloud family tests/test_gpu_frontend_edges.py runs on the device.

The oracle returns points, not chunks.  The chunk is made visible in its output: with a pure-translation velocity
(0, 0, v, 0, 0, 0) the rotation of every chunk is exactly the identity (first-order branch of expMapSO3 on a zero vector) and a
point with z = 0 comes out with z = v * t_k exactly, t_k the reference's own accumulated time of chunk k — tabulated the same
way (deskew_ref.times) and looked up bit for bit.

The census the GPU file relies on (every sparse cloud lags and has a rise of T_d - d, every straddle cloud lags on both sides of
the carry it is named for) is asserted here too, so a maker that stops producing such clouds fails without a GPU.
"""
import math

import numpy as np
import pytest

import deskew_ref as D
import oracle_lib as O
from mad_icp_amd import capi

HZ = 10.0


def _translation():
    T = np.eye(4)
    T[2, 3] = 0.37
    return np.eye(4), T


def chunks_from_z(out, vel):
    """walk-order chunks of a deskewed z = 0 cloud (rows in ascending azimuth) under the velocity (0, 0, v, 0, 0, 0)"""
    assert vel[2] != 0.0 and not vel[[0, 1, 3, 4, 5]].any()
    zt = vel[2] * D.times(HZ)
    assert np.unique(zt).size == zt.size
    table = {float(z): k for k, z in enumerate(zt)}
    return np.array([table[float(z)] for z in out[::-1, 2]], dtype=np.int64)   # KeyError: a z that is no chunk's


def oracle_chunks(pts):
    Tp, Tn = _translation()
    out, vel = O.deskew(pts, Tp, Tn, HZ)
    # x and y pass through untouched (identity rotation, zero translation): the rows are the input in azimuth order
    return chunks_from_z(out, vel), out


def check_against_oracle(pts):
    w = D.walk(pts)
    oc, out = oracle_chunks(pts)
    assert np.array_equal(out[:, :2], pts[w["order"], :2])       # the one possible order
    assert np.array_equal(w["chunks"], oc)
    Tp, Tn = _translation()
    for route in (0, 1):
        hout, hvel, _ = capi.host_deskew(pts, Tp, Tn, HZ, route=route)
        assert np.array_equal(chunks_from_z(hout, hvel), w["chunks"])
    return w


@pytest.mark.parametrize("kind", D.SPARSE_KINDS)
def test_sparse_clouds(kind):
    for n in D.SPARSE_SIZES:
        w = check_against_oracle(D.sparse_cloud(kind, n, z_zero=True))
        assert w["lagging"] >= 1, (kind, n)
        assert (w["rises"] >= 1) == D.sparse_has_rise(kind, n), (kind, n, w["rises"])
        # the census is a property of the azimuths alone: the same for the cloud the device gets (z drawn, not zero)
        w3 = D.walk(D.sparse_cloud(kind, n))
        assert np.array_equal(w3["chunks"], w["chunks"]) and np.array_equal(w3["T"], w["T"])


@pytest.mark.parametrize("P", sorted(D.STRADDLE_HEADS))
def test_straddle_clouds(P):
    w = check_against_oracle(D.straddle_cloud(P, z_zero=True))
    width = D.STRADDLE_HEADS[P]
    if P == 1024:                                        # the lag STARTS at the tile edge: the head itself does not lag there
        assert not w["lag"][1023] and w["lag"][1024] and 1024 in w["live_across"][D.TILE]
    else:
        assert w["lag_across"][width], (P, w["lagging"])
    if P != 54:  # (the sparse head of 54 starts below the first threshold: T_j - j >= 1 throughout, the clamp decides, and what
        # came before a wavefront edge does not matter; the other four cross 14 or 15 wavefront edges that do)
        assert w["live_across"][width] and len(w["live_across"][D.WAVE]) >= 14, (P, w["lagging"])


def test_table_end_clouds():
    for name, pts in D.table_end_clouds(z_zero=True).items():
        w = check_against_oracle(pts)
        if name == "last_three_chunks":
            assert np.array_equal(w["chunks"], np.arange(1, pts.shape[0] + 1)) and w["lagging"] == pts.shape[0]


def test_near_threshold_cloud():
    pts, near = D.near_threshold_cloud(z_zero=True)
    assert 380 <= near.sum() <= 420
    w = check_against_oracle(pts)
    # where the near points sit the walk has caught up: their chunk is their side of the threshold
    near_walk = near[w["order"]][::-1]
    assert np.array_equal(w["chunks"][near_walk], w["T"][near_walk])
    k = w["chunks"][near_walk]
    assert (np.diff(k)[::2] == 1).all()                  # the pair around one threshold: two different chunks


def _on_threshold_cloud():
    """the near-threshold cloud + points whose libm azimuth EQUALS a threshold: `<` stays in the chunk, `<=` would move on"""
    xy = D.on_threshold_points(count=40)
    assert xy.shape[0] >= 3
    pts, _ = D.near_threshold_cloud(z_zero=True)
    pts = np.vstack([pts, np.column_stack([xy, np.zeros(xy.shape[0])])])
    az = D.check_distinct(pts)
    on = np.isin(az, D.thresholds())
    assert on.sum() == xy.shape[0]
    return pts, on


def test_azimuths_exactly_on_a_threshold():
    pts, on = _on_threshold_cloud()
    w = check_against_oracle(pts)
    on_walk = on[w["order"]][::-1]
    assert np.array_equal(w["chunks"][on_walk], w["T"][on_walk])   # caught up there: the comparison alone decides


def test_the_walk_is_sensitive_to_its_comparison_and_its_start():
    """`<=` for `<`, or M_PI for M_PI - resolution, gives other chunks on clouds of this file — so the equalities above hold the
    reference's choice, not any walk."""
    pts, _ = _on_threshold_cloud()
    oc, _ = oracle_chunks(pts)
    assert np.array_equal(D.walk(pts)["chunks"], oc)
    assert not np.array_equal(D.walk(pts, strict=False)["chunks"], oc)
    assert not np.array_equal(D.walk(pts, first=math.pi)["chunks"], oc)
    for kind in D.SPARSE_KINDS:                             # the start of the table shows on every family
        sp = D.sparse_cloud(kind, 1025, z_zero=True)
        assert not np.array_equal(D.walk(sp, first=math.pi)["chunks"], oracle_chunks(sp)[0])
