"""tests/surfel_exact_ref.py held to itself: spectra known by hand (diagonal matrices, a known rotation of one, point sets whose
covariance is written down), the rank of hand-built cases, the certificate and the exact eigenvectors on numpy.linalg.eigh's own
pairs, the exact decision and the catalogue's placement.  No GPU, no native code."""
from fractions import Fraction

import numpy as np

import map_moments_ref as Mo
import surfel_exact_ref as X


def spectrum_of_points(w):
    return X.Spectrum(X.words(w))


def inside(sp, k, value):
    return sp.lo[k] <= value <= sp.hi[k]


def test_diagonal_spectra_by_hand():
    # points +-a, +-b, +-c on the axes about (1000, 1000, 1000): C = diag(2 a^2, 2 b^2, 2 c^2) / 6
    a, b, c = 300, 70, 9
    w = np.array([[a, 0, 0], [-a, 0, 0], [0, b, 0], [0, -b, 0], [0, 0, c], [0, 0, -c]]) + 1000
    sp = spectrum_of_points(w)
    assert sp.rank == 3
    for k, v in enumerate((c, b, a)):
        assert inside(sp, k, Fraction(2 * v * v, 6))
        assert float(sp.hi[k] - sp.lo[k]) <= 2.0 ** -90 * sp.lam[2]
    assert np.allclose(np.abs(sp.vector(0)), [0, 0, 1], atol=1e-15) and np.allclose(np.abs(sp.vector(2)), [1, 0, 0], atol=1e-15)
    # the same with b = c: a double root at the bottom, bracketed from both sides by the same interval
    w[4:] = np.array([[0, 0, b], [0, 0, -b]]) + 1000
    sp = spectrum_of_points(w)
    assert sp.rank == 3 and inside(sp, 0, Fraction(2 * b * b, 6)) and inside(sp, 1, Fraction(2 * b * b, 6))
    assert sp.lo[0] == sp.lo[1] and sp.hi[0] == sp.hi[1]


def test_a_known_rotation():
    # 3-4-5: the points +-(3, 4, 0) a and +-(-4, 3, 0) b and +-(0, 0, 5) c: C = (2 / 6) (25 a^2 u u^T + 25 b^2 v v^T + 25 c^2 z z^T)
    a, b, c = 40, 7, 2
    u, v, z = np.array([3, 4, 0]), np.array([-4, 3, 0]), np.array([0, 0, 5])
    w = np.array([a * u, -a * u, b * v, -b * v, c * z, -c * z]) + 5000
    sp = spectrum_of_points(w)
    for k, s in enumerate((c, b, a)):
        assert inside(sp, k, Fraction(2 * 25 * s * s, 6))
    assert np.allclose(np.abs(sp.vector(2)), [0.6, 0.8, 0.0], atol=1e-15)
    assert np.allclose(np.abs(sp.vector(1)), [0.8, 0.6, 0.0], atol=1e-15)
    assert np.allclose(np.abs(sp.vector(0)), [0.0, 0.0, 1.0], atol=1e-15)


def test_rank_by_hand():
    assert spectrum_of_points([[5, 6, 7]] * 9).rank == 0
    assert spectrum_of_points([[5, 6, 7]]).rank == 0
    assert spectrum_of_points([[0, 0, 0], [1, 0, 0]]).rank == 1
    assert spectrum_of_points([[k * 5, k * 3, k] for k in range(50)]).rank == 1
    assert spectrum_of_points([[0, 0, 0], [65535, 65535, 65535], [65535, 65535, 65535]]).rank == 1
    assert spectrum_of_points([[0, 0, 0], [1, 0, 0], [0, 1, 0]]).rank == 2
    assert spectrum_of_points([[x, y, x + y] for x in range(5) for y in range(7)]).rank == 2
    assert spectrum_of_points([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]).rank == 3
    line = [[k * 5, k * 3, k] for k in range(50)]
    assert spectrum_of_points(line + [[0, 0, 1]]).rank == 2 and spectrum_of_points(line + [[0, 0, 1], [1, 0, 0]]).rank == 3
    sp = spectrum_of_points(line)
    assert sp.lo[0] == sp.hi[0] == sp.lo[1] == sp.hi[1] == 0 and sp.lo[2] > 0  # (what the rank says is zero is exactly zero)


def test_counting_below():
    A = [[2, 0, 0], [0, 2, 0], [0, 0, 5]]
    inv = X.invariants(A)
    assert inv == (9, 24, 20)
    assert [X._below(inv, j, 1) for j in (0, 1, 2, 3, 5, 6)] == [0, 0, 0, 2, 2, 3]
    assert X._below(X.invariants([[0] * 3] * 3), 0, 1) == 0 and X._below(X.invariants([[0] * 3] * 3), 1, 1) == 3


def test_certificates_of_eigh():
    """numpy.linalg.eigh's own pairs on random populations: the residual is rounding, Weyl's interval holds an exact eigenvalue, and
    the exact eigenvector is within Davis-Kahan's bound of eigh's"""
    rng = np.random.default_rng(3)
    for trial in range(40):
        n = int(rng.integers(4, 60))
        scale = np.array([rng.integers(1, 30000), rng.integers(1, 3000), rng.integers(1, 300)])
        w = (rng.integers(0, 2, size=(n, 3)) * scale + rng.integers(0, scale + 1, size=(n, 3))) % 65536
        M = X.words(w)
        sp = X.Spectrum(M)
        lam, V = np.linalg.eigh(Mo.covariances(np.array([M], np.uint64))[0])
        s2 = (X.VOXEL / 65536.0) ** 2
        for k in range(3):
            resid, vv, claimed = sp.certificate(lam[k] * s2, V[:, k])
            assert abs(float(vv) - 1.0) <= 1e-14
            assert resid <= 1e-13 * sp.lam[2] + 100 * sp.floor, (trial, k, resid)
            assert sp.lo[k] - Fraction(resid) * 2 <= claimed <= sp.hi[k] + Fraction(resid) * 2  # Weyl (x2: the fp64 of resid)
            gap = sp.gap((k,), claimed)
            if gap >= 1e-6 * sp.lam[2]:
                sine = float(np.linalg.norm(np.cross(V[:, k], sp.vector(k))))
                assert sine <= resid / gap + 1e-14, (trial, k, sine, resid / gap)
    # a wrong pair is told: eigenvector 1 claimed for eigenvalue 0
    resid, _, _ = sp.certificate(lam[0] * s2, V[:, 1])
    assert resid >= 0.99 * (lam[1] - lam[0])


def test_exact_decision():
    plane = spectrum_of_points([[x * 100, y * 100, 0] for x in range(5) for y in range(3)])  # lambda = 0, 2/3 1e4, 2 1e4
    assert plane.rank == 2 and inside(plane, 1, Fraction(20000, 3)) and inside(plane, 2, Fraction(20000))
    assert plane.inlier(3, 1.0) and plane.inlier(15, 1e-3) and not plane.inlier(16, 1.0)
    line = spectrum_of_points([[k, k, 7] for k in range(10)])
    assert not line.inlier(3, 1.0) and line.decisive(1.0, 1e300)
    box = spectrum_of_points([[x * 100, y * 40, z * 10] for x in range(2) for y in range(2) for z in range(2)])  # 2500, 400, 25
    assert box.inlier(3, 1.0) and box.inlier(3, 0.3) and not box.inlier(3, 1e-3) and box.inlier(3, 0.0626) and box.inlier(3, 0.0624) is False
    assert box.inlier(3, 0.0625) is None  # (25 = 0.0625 x 400 exactly: on the threshold, which brackets cannot tell)
    assert box.decisive(0.3, 1.0) and not box.decisive(0.0625, 1.0) and not box.decisive(0.3, 300.0)
    cube = spectrum_of_points([[x, y, z] for x in (0, 9) for y in (0, 9) for z in (0, 9)])  # a triple root
    assert cube.inlier(3, 1.0) and cube.inlier(3, 0.3) is False


def test_placement_is_exact():
    """every entry's points are exact doubles in its own cell whose quantised offsets are the intended integers, the cells are all
    different, and both ends of the key range and a negative cell are there"""
    cat = X.catalogue()
    for e in cat[:40] + cat[-4:]:
        q = e.points()
        assert np.array_equal(np.floor(q / X.VOXEL), np.tile(np.array(e.cell, np.float64), (e.n, 1)))
        assert np.array_equal(Mo.offsets(q, X.VOXEL), e.w)
        p = e.probe()
        assert np.array_equal(np.floor(p / X.VOXEL), np.array(e.cell, np.float64))
    cells = {e.cell for e in cat}
    assert len(cells) == len(cat)
    assert {(-(1 << 20),) * 3, ((1 << 20) - 1,) * 3, (-1, -1, -1)} <= cells
    assert cat[0].key == 0 and cat[1].key == 2 ** 63 - 1
    names = {e.name.split("/")[0] for e in cat}
    assert {"identical3", "identical4096", "line_axis3", "line_face100", "line_531_100", "line_531_jitter", "plane_axis", "plane_tilted",
            "plane_floored", "square", "cube", "uniform4096", "noisy_plane_1e-2", "noisy_plane_1e-4", "noisy_plane_1e-6", "top_cube_100000",
            "top_thin_plane_100000", "three_and_one", "one", "two", "triangle", "tetra"} <= names
