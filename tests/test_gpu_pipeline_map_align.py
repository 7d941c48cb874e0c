"""Pipeline.mapRegister / mapLinearize — registering a scan against the voxel map's surfels where the map lives — on the 8-frame
16 x 450 drive of tests/test_gpu_pipeline_registered_scan.py, both front-ends, against the restatement of tests/map_align_ref.py
fed mapCloud / mapKeys / mapSurfels of that moment: the linearise-only form exactly (counts, row, e; H, b, chi2 by value), every
traced round's sums exactly at the pipeline's own X_k, the steps within tests/test_gpu_gn_step.py's tolerance, the closing
linearisation in info; the map and the pipeline's pose untouched; the errors by exception type."""
import numpy as np
import pytest

import gn_step_ref as G
import map_align_ref as A
from test_gpu_pipeline_registered_scan import bits, drive, feed, pipeline  # noqa: F401  (drive: the module-scoped fixture)

pytestmark = pytest.mark.gpu

VOXEL = 0.5
PARAMS = dict(reach=1, max_dist=0.45, rho=0.05, min_count=4, flat=0.5)


def columns(p):
    return p.mapCloud(), p.mapKeys(), p.mapSurfels()


def everything(p):
    return [c.tobytes() for c in (p.mapCloud(), p.mapKeys(), p.mapMoments()) + tuple(p.mapSurfels())]


def offset(T):
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = A.OFFSET
    return T @ D


def same(info, want, rows=True):
    assert np.array_equal(info["counts"], want["counts"]), (info["counts"], want["counts"])
    assert np.array_equal(info["H"], want["H"]) and np.array_equal(info["b"], want["b"]) and info["chi2"] == want["chi2"]
    if rows:
        assert info["row"].dtype == np.int32 and np.array_equal(info["row"], want["row"]) and info["e"].tobytes() == want["e"].tobytes()


@pytest.mark.parametrize("device_frontend", [True, False])
def test_register_and_linearize_by_hand(natives, drive, device_frontend):
    p = pipeline(False, device_frontend)
    probe = drive[1]["pts"]
    with pytest.raises(RuntimeError):
        p.mapRegister(probe, np.eye(4), 1)  # accumulation is off
    p.setMapAccumulation(VOXEL)
    with pytest.raises(RuntimeError):
        p.mapLinearize(probe, np.eye(4))  # no moments
    p.setMapAccumulation(VOXEL, moments=1 << 20)
    T0 = offset(np.eye(4))
    pose, info = p.mapRegister(probe, T0, 2, trace=True)  # no frame folded yet: an empty map
    assert np.array_equal(pose, T0) and not info["H"].any() and not info["b"].any() and info["chi2"] == 0.0
    assert np.array_equal(info["counts_rounds"], np.tile(np.array([probe.shape[0], 0, 0, 0], np.uint64), (3, 1)))
    pose, info = p.mapLinearize(probe[:0], T0, with_rows=True)
    assert np.array_equal(pose, T0) and not info["counts"].any() and info["row"].shape == (0,) and info["e"].shape == (0,)
    for i, f in enumerate(drive[:4]):
        feed(p, "cloud", i, f)
    T = np.asarray(p.currentPose())
    rows, keys, surfels = columns(p)
    before = everything(p)
    c = 8.0 * G.rho_ref()
    for cloud, start in ((drive[3]["pts"], offset(T)), (drive[0]["pts"][:333], offset(np.eye(4)))):
        R0, t0 = start[:3, :3], np.array(start[:3, 3])
        for params in (dict(), PARAMS, dict(PARAMS, reach=0)):
            want = A.linearize(rows, keys, surfels, cloud, R0, t0, VOXEL, **dict(A.DEFAULT, **params))
            pose, info = p.mapLinearize(cloud, start, with_rows=True, **params)
            assert np.array_equal(pose, start)
            same(info, want)
            same(p.mapLinearize(cloud, start, **params)[1], want, rows=False)
            assert want["counts"][3] > 50
            pose, info = p.mapRegister(cloud, start, 3, trace=True, **params)
            assert np.array_equal(info["X"][0], np.concatenate([R0.reshape(-1), t0]))
            for k in range(4):
                Rk, tk = info["X"][k][:9].reshape(3, 3), info["X"][k][9:]
                lin = A.linearize(rows, keys, surfels, cloud, Rk, tk, VOXEL, **dict(A.DEFAULT, **params))
                assert np.array_equal(info["counts_rounds"][k], lin["counts"]) and np.array_equal(info["H_rounds"][k], lin["H"]), k
                assert np.array_equal(info["b_rounds"][k], lin["b"]) and info["chi2_rounds"][k] == lin["chi2"], k
                if k < 3:
                    Rn, tn = A.step(lin["H"], lin["b"], Rk, tk)
                    _, _, tol = G.bounds(G.step(lin["H"], lin["b"], info["X"][k]), info["X"][k], c)
                    assert np.all(np.abs(info["X"][k + 1] - np.concatenate([Rn.reshape(-1), tn])) <= tol), k
            assert np.array_equal(pose[:3, :3].reshape(-1), info["X"][3][:9]) and np.array_equal(pose[:3, 3], info["X"][3][9:])
            assert np.array_equal(pose[3], [0.0, 0.0, 0.0, 1.0])
            assert np.array_equal(info["H"], info["H_rounds"][3]) and info["chi2"] == info["chi2_rounds"][3]
            assert info["chi2_rounds"][1] < info["chi2_rounds"][0] and not np.array_equal(info["X"][1], info["X"][0])
            plain_pose, plain = p.mapRegister(cloud, start, 3, **params)
            assert np.array_equal(plain_pose, pose) and set(plain) == {"H", "b", "chi2", "counts"} and np.array_equal(plain["H"], info["H"])
    assert everything(p) == before                                            # the map is only read ...
    assert np.array_equal(bits(np.asarray(p.currentPose())), bits(T))         # ... and the pipeline's pose is not the call's business
    bad_T = T.copy()
    bad_T[1, 3] = np.nan
    for args, kw in (((probe, bad_T, 1), {}), ((probe, T, -1), {}), ((probe, T, 65), {}), ((probe[:, :2], T, 1), {}), ((probe, T[:3], 1), {}),
                     ((probe, T, 1), dict(reach=2)), ((probe, T, 1), dict(max_dist=-1.0)), ((probe, T, 1), dict(max_dist=np.nan)),
                     ((probe, T, 1), dict(rho=0.0)), ((probe, T, 1), dict(rho=np.nan)), ((probe, T, 1), dict(min_count=2)),
                     ((probe, T, 1), dict(flat=0.0)), ((probe, T, 1), dict(flat=1.5))):
        with pytest.raises(ValueError):
            p.mapRegister(*args, **kw)
        if len(args[0].shape) == 2 and args[2] == 1:
            with pytest.raises(ValueError):
                p.mapLinearize(args[0], args[1], **kw)
    assert everything(p) == before



@pytest.mark.parametrize("device_frontend", [True, False])
def test_drive_with_the_observer_on_and_off(natives, drive, device_frontend):
    """setMapAlignment(True): every folded frame reports mapRegister of its own cloud from its own pose against the map as it stood
    before the fold; poses, keyframe decisions and every map column are the same bits with the option on and off."""
    on, off = pipeline(False, device_frontend), pipeline(False, device_frontend)
    for p in (on, off):
        p.setMapAccumulation(VOXEL, moments=1 << 20)
    on.setMapAlignment(True, 3, **PARAMS)
    assert on.mapFrameAlignment() is None and off.mapFrameAlignment() is None
    inliers = 0
    for i, f in enumerate(drive[:5]):
        before = columns(on) if on.mapSize() else None
        for p in (on, off):
            feed(p, "cloud", i, f)
        assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(off.currentPose()))), i
        assert on.keyframeID() == off.keyframeID() and on.isMapUpdated() == off.isMapUpdated(), i
        assert everything(on) == everything(off), i
        assert off.mapFrameAlignment() is None
        pose, info = on.mapFrameAlignment()
        T = np.asarray(on.currentPose())
        if before is None:                                                # the first frame met an empty map
            assert np.array_equal(pose, T) and not info["H"].any() and not info["counts"][1:].any() and info["counts"][0] == f["pts"].shape[0]
            continue
        rows, keys, surfels = before
        R, t, lins, _ = A.register(rows, keys, surfels, f["pts"], T[:3, :3], np.array(T[:3, 3]), 3, VOXEL, **PARAMS)
        assert np.array_equal(info["counts_start"], lins[0]["counts"]) and info["chi2_start"] == lins[0]["chi2"], i
        dt, da = A.pose_distance(pose[:3, :3], pose[:3, 3], R, t)
        assert dt <= 1e-5 and da <= 1e-5, (i, dt, da)
        here = A.linearize(rows, keys, surfels, f["pts"], pose[:3, :3], np.array(pose[:3, 3]), VOXEL, **PARAMS)
        assert np.array_equal(info["counts"], here["counts"]) and np.array_equal(info["H"], here["H"]) and info["chi2"] == here["chi2"], i
        assert info["iterations"] == 3
        inliers += int(info["counts"][3])
    assert inliers > 1000
    assert np.array_equal(bits(np.asarray(on.trajectory())), bits(np.asarray(off.trajectory())))
    on.setMapAlignment(False)
    assert on.mapFrameAlignment() is None
    for args, kw in (((True, 65), {}), ((True, -1), {}), ((True, 3), dict(reach=2)), ((True, 3), dict(min_count=1)), ((True, 3), dict(flat=2.0)),
                     ((True, 3), dict(rho=-1.0)), ((True, 3), dict(max_dist=np.nan))):
        with pytest.raises(ValueError):
            on.setMapAlignment(*args, **kw)
    plain = pipeline(False, device_frontend)
    plain.setMapAccumulation(VOXEL)
    with pytest.raises(RuntimeError):
        plain.setMapAlignment(True)                                       # the map has no moments
