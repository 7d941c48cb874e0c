"""The host twin's surfels (madicp_host_map_download_surfels: csrc/common/voxel_moments.h's map_surfel over csrc/common/eig3.h's
closed-form eig3_sym) and the gate that stands on them (madicp_host_map_register: csrc/common/map_align.h's align_inlier) against
the EXACT integer reference of tests/surfel_exact_ref.py, over its catalogue of voxel populations: identical and collinear points,
exact and noisy planes, double and triple roots, offsets at the top of the voxel where S2 / n - m m cancels, n = 100 000, every
column choice and ordering inside the solver, cells at both ends of the key range.  No GPU.  The checks are functions of (rows,
words, surfels, a register call), so tests/test_gpu_map_surfels_exact.py holds the device to the same reference with them.

MEASURED here, host twin against the exact reference over the catalogue's 741 rows (669 of them with n >= 3), and asserted TENFOLD:
  eigenvalues   |eig_i - lambda_i| <= a lambda2 + c floor, floor = 2^-52 max(S2_aa / n) s^2:
                a = 4.77e-8 over the rows whose floor is below 1e-10 lambda2 (the float32 rounding of the output, 2^-24 = 5.96e-8 at
                most), c = 0.40 over the others (100 000 points within three steps of the voxel's top corner); asserted 4.77e-7, 4.0
  normals       where lambda1 - lambda0 >= 1e-3 lambda2 (331 rows): the sine of the angle to the exact eigenvector 2.46e-8 (the
                float32 rounding of three components), asserted 2.46e-7 + 10 c floor / (lambda1 - lambda0) — the cancellation moves
                the vectors as it moves the values — and never above the certificate's Davis-Kahan bound
  lines         where lambda2 - lambda1 >= 1e-3 lambda2 but lambda1 - lambda0 is not (264 rows): |normal . v2| 1.56e-8, asserted
                1.56e-7 + 10 c floor / (lambda2 - lambda1) and Davis-Kahan's bound for the span of v0 and v1
  unit length   | ||normal||^2 - 1 | 7.3e-8; asserted 2 sqrt(3) 2^-25 = 1.03e-7, the float32 rounding of three components
  the solver    WITHOUT the zero rule (voxel_moments.h: surfel_solve), its error on an eigenvalue that is exactly zero is at most
                3.73e-9 of lambda2 — measured again by tests/cpp/map_surfel_check.cpp at every run of
                tests/test_map_surfel_sanitized.py, which prints it — and the cancellation 0.43 floors at the worst (the c above,
                with a's share left in): what kSurfelZeroShare = 2^-24 and kSurfelZeroFloor = 4 are sixteen and nine times of
Without the zero rule the rank-1 gate assertions below fail on the collinear entries (eig1 = +6e-11 > 0 admits a line).
No benchmark path computes a surfel; bench.py --gpus 1 --steps 200 --warmup 20 on one MI355X gave 4755.6 registrations/s before the
rule and, with it, 4717.2 .. 4776.6 in eight runs over three visits (4718.1, 4776.6, 4771.7, 4717.2, 4724.6, 4721.3, 4721.2, 4721.7):
the runs fall into two groups about 1 % apart, and the one figure from before lies between them."""
import math

import numpy as np
import pytest

import cloud_export_ref as E
import map_align_ref as A
import map_moments_ref as Mo
import surfel_exact_ref as X
from mad_icp_amd import capi

MEASURED_A = 4.77e-8
MEASURED_C = 0.40
MEASURED_ANGLE = 2.46e-8
MEASURED_LINE = 1.56e-8
NEGLIGIBLE_FLOOR = 1e-10  # a row's floor / lambda2 below which its whole error is charged to `a`
FLATS = (1.0, 0.3, 1e-3)
NORM2_BOUND = 2 * math.sqrt(3.0) * 2.0 ** -25 + 1e-12  # | ||v + d||^2 - 1 | <= 2 ||v|| ||d|| + ||d||^2, |d_i| <= 2^-25, fp64 ||v|| = 1
# the rows left out of the gate's comparison as NOT DECISIVE, by the catalogue name they start with, and their exact margin: the
# line with one unit of jitter has exact rank 3 — a plane exists — with lambda1 / lambda2 = 1.78e-8, below the zero rule's 5.96e-8
NOT_DECISIVE = {"line_531_jitter": "lambda1 / lambda2 = 1.78e-8: rank 3, thinner than the solver can tell from a line"}


def asserted(sp):
    """the bound on an eigenvalue's error that is ASSERTED, in offset units squared"""
    return sp.error(10 * MEASURED_A, 10 * MEASURED_C)


def decisive(sp):
    """further from every threshold of the gate, at every flat tried, than the asserted error plus the zero rule's own threshold"""
    err = asserted(sp) + sp.error(A.ZERO_SHARE, A.ZERO_FLOOR)
    return all(sp.decisive(flat, err) for flat in FLATS)


def min_counts(rows):
    """3, n and n + 1 of every population size there is (what is legal of them)"""
    return sorted({3} | {c for e in rows for c in (e.n, e.n + 1) if c >= 3})


def fold(m):
    """the catalogue folded into map m (anything with insert / download_keys / download_moments on clouds given as arrays); the
    entries in row order, after the PRECONDITION that every row's ten words are the intended integers"""
    I, z = E.IDENTITY
    added, size = m.insert(X.cloud(), I, z)
    assert added == size == len(X.catalogue())
    return rows_of(m.download_keys(), m.download_moments())


def rows_of(keys, mom):
    rows = X.by_row(keys)
    assert mom.shape == (len(rows), 10)
    for r, e in enumerate(rows):
        assert mom[r].tolist() == e.M, e.name
    return rows


def check_surfels(rows, keys, mom, surfels, tag):
    """section by section what the module docstring says, on one side's surfels; returns the measured figures"""
    c, nrm, eig, cnt = surfels
    assert c.dtype == nrm.dtype == eig.dtype == np.float32 and cnt.dtype == np.uint32
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(nrm)) and np.all(np.isfinite(eig))
    assert cnt.tolist() == [e.n for e in rows]
    assert E.same_bits(c, Mo.centroids(mom, keys, X.VOXEL))
    assert np.all(eig[:, 0] <= eig[:, 1]) and np.all(eig[:, 1] <= eig[:, 2])
    assert not np.any(np.signbit(eig))  # (+0.0 or positive: the zero rule)
    n2 = np.sum(nrm.astype(np.float64) ** 2, axis=1)
    assert np.all(nrm[cnt < 3] == 0.0)
    worst_norm = float(np.abs(n2[cnt >= 3] - 1.0).max())
    # eigenvalues
    err, l2, fl = X.eig_errors(rows, eig)
    worst = err.max(axis=1)
    small = (l2 > 0) & (fl <= NEGLIGIBLE_FLOOR * l2)
    a = float((worst[small] / l2[small]).max())
    rest = ~small & (fl > 0)
    c_meas = float((np.maximum(worst[rest] - MEASURED_A * l2[rest], 0.0) / fl[rest]).max())
    assert np.all(worst[~small & ~rest] == 0.0)  # (a floor of zero: every point at offset 0, the spectrum is 0, 0, 0)
    # the zero rule: what is delivered is +0.0 or above the threshold (to the rounding of the delivery)
    s2 = (X.VOXEL / 65536.0) ** 2
    e64 = eig.astype(np.float64) / s2
    at = A.zero_at(mom, e64[:, 2])
    assert np.all((e64 == 0.0) | (e64 > at[:, None] * (1 - 2.0 ** -22)))
    # ... and from the other side, on the EXACT spectrum: an eigenvalue clearly above the threshold (1.5 times: the solver's error
    # is a sixteenth of the share) is not zeroed — a share too large would show here, on the thin planes — one clearly below is
    lam = np.array([e.spectrum.lam for e in rows])
    at_exact = A.zero_at(mom, lam[:, 2])[:, None]
    above, below = lam > 1.5 * at_exact, lam < 0.5 * at_exact
    assert np.all(e64[above] != 0.0), (tag, [rows[r].name for r in np.argwhere(above & (e64 == 0.0))[:4, 0]])
    assert np.all(e64[below] == 0.0), (tag, [rows[r].name for r in np.argwhere(below & (e64 != 0.0))[:4, 0]])
    near = np.count_nonzero(above & (lam < 2.0 * at_exact))
    assert near >= 36  # (witnesses within a factor of two of the threshold: eig0 of the noisy planes at 1e-4, 1.98 times it)
    # normals
    angle = line = 0.0
    n_angle = n_line = 0
    for r, e in enumerate(rows):
        sp = e.spectrum
        if e.n < 3 or sp.lam[2] <= 0:
            continue
        v = nrm[r].astype(np.float64)
        plane = sp.lam[1] - sp.lam[0] >= 1e-3 * sp.lam[2]
        pencil = not plane and sp.lam[2] - sp.lam[1] >= 1e-3 * sp.lam[2]
        if not (plane or pencil):
            continue
        resid, vv, lam = sp.certificate(eig[r, 0], nrm[r])
        dk = resid / sp.gap((0,) if plane else (0, 1), lam)
        # (the cancellation in C moves the eigenvectors by its size over the gap, as it moves the eigenvalues by its size)
        cancel = 10 * MEASURED_C * sp.floor / ((sp.lam[1] - sp.lam[0]) if plane else (sp.lam[2] - sp.lam[1]))
        if plane:
            got = float(np.linalg.norm(np.cross(v, sp.vector(0))) / math.sqrt(float(vv)))
            if cancel <= MEASURED_ANGLE:
                angle = max(angle, got)
            n_angle += 1
            assert got <= 10 * MEASURED_ANGLE + cancel, (tag, e.name, got)
        else:
            got = float(abs(v @ sp.vector(2)) / math.sqrt(float(vv)))
            if cancel <= MEASURED_LINE:
                line = max(line, got)
            n_line += 1
            assert got <= 10 * MEASURED_LINE + cancel, (tag, e.name, got)
        assert got <= dk + 1e-12, (tag, e.name, got, dk)  # (1e-12: the fp64 of `got` itself)
    got = dict(a=a, c=c_meas, angle=angle, line=line, norm=worst_norm, planes=n_angle, lines=n_line)
    print("%s: rows %d (n >= 3: %d); eigenvalues a = %.3e of lambda2, c = %.3f floors; normals %.3e rad over %d rows, lines %.3e over %d"
          " rows; | ||n||^2 - 1 | %.3e" % (tag, len(rows), int(np.count_nonzero(cnt >= 3)), a, c_meas, angle, n_angle, line, n_line, worst_norm))
    assert n_angle >= 200 and n_line >= 100
    assert worst_norm <= NORM2_BOUND
    for r, e in enumerate(rows):
        assert worst[r] <= asserted(e.spectrum), (tag, e.name, worst[r], asserted(e.spectrum))
    return got


def check_gate(rows, stored, keys, surfels, register, tag):
    """register(cloud, min_count, flat) -> a linearise-only answer with per-point outputs.  One probe per row, at its fp64 centroid,
    reach 0: the probe's row is its own voxel's.  On every decisive row the decision is the exact one; the side's row, e, counts and
    sums are map_align_ref.linearize's on the side's own surfels."""
    I, z = E.IDENTITY
    probes = np.array([e.probe() for e in rows])
    seen = {True: 0, False: 0}
    for min_count in min_counts(rows):
        for flat in FLATS:
            at = (tag, min_count, flat)
            got = register(probes, min_count, flat)
            want = A.linearize(stored, keys, surfels, probes, I, z, X.VOXEL, reach=0, min_count=min_count, flat=flat)
            assert want["row"].tolist() == list(range(len(rows))), at
            assert got["row"].tolist() == want["row"].tolist(), at
            assert got["counts"][0].tolist() == want["counts"].tolist(), at
            assert got["e"].tobytes() == want["e"].tobytes(), at
            assert got["H"][0].tobytes() == want["H"].tobytes() and got["b"][0].tobytes() == want["b"].tobytes(), at
            assert float(got["chi2"][0]) == want["chi2"], at
            for r, e in enumerate(rows):
                sp = e.spectrum
                if sp.rank <= 1:
                    assert not want["inlier"][r], at + (e.name, "no plane exists in a voxel of rank %d" % sp.rank)
                elif decisive(sp):
                    exact = sp.inlier(min_count, flat)
                    assert exact is not None and bool(want["inlier"][r]) == exact, at + (e.name, exact)
                    seen[exact] += 1
                    if sp.lam[0] == 0.0 and e.n >= min_count:
                        assert want["inlier"][r], at + (e.name, "an exact plane")
    assert seen[True] >= 1000 and seen[False] >= 1000
    return seen


# ---- the reference alone ---------------------------------------------------------------------------------------------------------------
def test_every_branch_of_the_solver_is_reached():
    """the CENSUS: every column choice of kernel_vector, both cross-product picks, both k/l orders, the double-root branch and the
    identity branch of eig3_sym are reached, with margin, by at least one entry"""
    reached = {}
    for e in X.catalogue():
        for b in X.branches(e.spectrum):
            reached[b] = reached.get(b, 0) + 1
    print(sorted(reached.items()))
    assert set(reached) == X.ALL_BRANCHES
    assert len(X.catalogue()) > 512 and sum(e.n for e in X.catalogue()) < 300000
    ranks = {e.spectrum.rank for e in X.catalogue()}
    assert ranks == {0, 1, 2, 3}


def test_the_rows_left_out_are_the_named_ones_and_few():
    full = [e for e in X.catalogue() if e.n >= 3]
    out = [e for e in full if not decisive(e.spectrum)]
    for e in out:
        print("%-40s rank %d, lambda1 / lambda2 = %.3e, |lambda0 - flat lambda1| / lambda2 = %s" % (
            e.name, e.spectrum.rank, e.spectrum.margin(1.0)[0], ["%.3e" % e.spectrum.margin(f)[1] for f in FLATS]))
    print("left out %d of %d" % (len(out), len(full)))
    assert {e.name.split("/")[0] for e in out} == set(NOT_DECISIVE)
    assert len(out) <= 0.10 * len(full)
    assert all(e.spectrum.rank >= 2 for e in out)  # (rank <= 1 is never left out)


# ---- the host twin ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(natives):
    m = capi.HostMap.create(X.VOXEL, 64, 1 << 24, False, None, 1 << 20)
    rows = fold(m)
    yield m, rows
    m.close()


def test_surfels_against_the_exact_reference(twin):
    m, rows = twin
    check_surfels(rows, m.download_keys(), m.download_moments(), m.download_surfels(), "host twin")  # (prints what it measures)


def test_the_gate_decides_as_the_exact_spectrum_would(twin):
    m, rows = twin
    I, z = E.IDENTITY
    seen = check_gate(rows, m.download_f32(), m.download_keys(), m.download_surfels(),
                      lambda cloud, mc, flat: m.register(cloud, I, z, 0, reach=0, min_count=mc, flat=flat, per_point=True), "host twin")
    print("decisive decisions: %d inliers, %d refused" % (seen[True], seen[False]))


def test_windows_of_the_surfels(twin):
    m, rows = twin
    full = m.download_surfels()
    for first in (0, 255, 256, 257, len(rows) - 1):
        for a, b in zip(m.download_surfels(first), full):
            assert a.tobytes() == b[first:].tobytes(), first
