"""The device map's surfels (madicp_map_download_surfels: fe::map_surfels, one lane per row through csrc/common/voxel_moments.h's
map_surfel) and the gate of madicp_map_register_cloud that stands on them, held DIRECTLY to the exact integer reference of
tests/surfel_exact_ref.py over its catalogue of degenerate voxel populations — with the checks and the tenfold-measured bounds of
tests/test_host_map_surfels_exact.py, not only through the host twin, which is the same source.  The catalogue is 741 rows, so
fe::map_surfels' 256-lane blocks see two full blocks and a partial one, and windows that start at rows 0, 255, 256, 257 and at the
last row.  Moments and centroids are bit-equal to the twin's; eigenvalues within 4 float32 ulps and normals within 2.4e-7 of it.
The device's atan2 / cos / sin may differ from libm's in the last bit: a decisive row is by construction further from every
threshold than that."""
import numpy as np
import pytest

import cloud_export_ref as E
import map_align_ref as A
import map_moments_ref as Mo
import surfel_exact_ref as X
import test_host_map_surfels_exact as H
from map_impls import maps  # noqa: F401 (maps is a fixture)
from test_gpu_map_moments import ulps

pytestmark = pytest.mark.gpu

SPEC = dict(voxel=X.VOXEL, initial_rows=64, max_rows=1 << 24, with_attr=False, max_count=1 << 20)


@pytest.fixture
def folded(ctx, maps):
    """(device map, host twin, the catalogue's entries in row order) after one fold of the whole catalogue into both"""
    d, h = maps.dev(ctx, **SPEC), maps.host(**SPEC)
    I, z = E.IDENTITY
    pts = X.cloud()
    for m in (d, h):
        assert tuple(m.insert(pts, I, z)) == (len(X.catalogue()),) * 2
    return d, h, H.rows_of(d.keys(), d.moments())


def register(m):
    I, z = E.IDENTITY
    return lambda cloud, min_count, flat: m.register(cloud, I, z, 0, reach=0, min_count=min_count, flat=flat, per_point=True)


def test_moments_and_centroids_are_the_twins_bits(folded):
    d, h, rows = folded
    assert d.keys().tobytes() == h.keys().tobytes() and d.moments().tobytes() == h.moments().tobytes()
    assert E.same_bits(d.rows(), h.rows())
    (c, _, _, cnt), (hc, _, _, hcnt) = d.surfels(), h.surfels()
    assert c.dtype == np.float32 and E.same_bits(c, hc) and cnt.dtype == np.uint32 and cnt.tobytes() == hcnt.tobytes()


def test_surfels_against_the_exact_reference(folded):
    d, _, rows = folded
    H.check_surfels(rows, d.keys(), d.moments(), d.surfels(), "device")


def test_surfels_against_the_host_twin_on_decisive_rows(folded):
    d, h, rows = folded
    (_, nrm, eig, _), (_, hn, he, _) = d.surfels(), h.surfels()
    decisive = np.array([H.decisive(e.spectrum) for e in rows])
    assert np.count_nonzero(decisive) >= 0.9 * len(rows)
    # EVERY eigenvalue of every decisive row, but for one on the zero rule's threshold itself: the two sides' solves differ by the
    # last bit of atan2 / cos / sin, some 1e-16 of w2, so only an eigenvalue that the TWIN computes within 1e-6 of the threshold
    # (ten orders more than that difference) may be +0.0 on one side and not on the other.  The catalogue has none.
    s2 = (X.VOXEL / 65536.0) ** 2
    h64 = he.astype(np.float64) / s2
    at = A.zero_at(d.moments(), h64[:, 2])[:, None]
    on_threshold = (h64 != 0.0) & (np.abs(h64 - at) <= 1e-6 * at)
    clear = decisive[:, None] & ~on_threshold
    print("eigenvalues compared: %d of %d on decisive rows" % (np.count_nonzero(clear), 3 * np.count_nonzero(decisive)))
    assert np.count_nonzero(on_threshold) == 0 and np.count_nonzero(clear) == 3 * np.count_nonzero(decisive)
    assert np.array_equal((eig == 0.0)[clear], (he == 0.0)[clear])
    worst_ulps = int(ulps(eig[clear], he[clear]).max())
    gap = decisive & np.array([e.n >= 3 and e.spectrum.lam[1] - e.spectrum.lam[0] >= 1e-3 * e.spectrum.lam[2] for e in rows])
    worst = float(Mo.sign_free_diff(nrm[gap], hn[gap]).max())
    print("eigenvalues %d ulps, normals %.3e over %d rows" % (worst_ulps, worst, np.count_nonzero(gap)))
    assert np.count_nonzero(gap) >= 200
    assert worst_ulps <= 4
    assert worst <= 2.4e-7


def test_windows_of_the_surfels(folded):
    d, _, rows = folded
    full = d.surfels()
    for first in (0, 255, 256, 257, len(rows) - 1):
        got = d.surfels(first)
        assert got[0].shape[0] == len(rows) - first
        for a, b in zip(got, full):
            assert a.dtype == b.dtype and a.tobytes() == b[first:].tobytes(), first


def test_the_gate_decides_as_the_exact_spectrum_would(folded):
    """row, e, counts, H, b and chi2 are map_align_ref.linearize's on the device's own surfels, whose decisions are the exact ones"""
    d, _, rows = folded
    seen = H.check_gate(rows, d.rows(), d.keys(), d.surfels(), register(d), "device")
    print("decisive decisions: %d inliers, %d refused" % (seen[True], seen[False]))


def test_the_same_call_twice_gives_the_same_bits(folded):
    d, _, rows = folded
    probes = np.array([e.probe() for e in rows])
    one, two = register(d)(probes, 3, 0.3), register(d)(probes, 3, 0.3)
    assert sorted(one) == sorted(two)
    for k in one:
        assert np.asarray(one[k]).tobytes() == np.asarray(two[k]).tobytes(), k
    assert int(one["counts"][0, 3]) > 0
