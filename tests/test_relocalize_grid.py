"""mad_icp_amd.relocalize.pose_grid: the hypotheses Pipeline.mapScorePoses / mapRelocalize are fed — size, order, the centre first,
rigid transforms, zero extents.  Plain numpy, no library, no GPU."""
import numpy as np
import pytest

import cloud_export_ref as E
from mad_icp_amd.relocalize import pose_grid


def centre(seed=3):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = E.random_pose(seed)
    return T


def test_size_and_the_centre_first():
    C = centre()
    G = pose_grid(C, 1.0, 0.5, np.deg2rad(20.0), 2)
    assert G.shape == (5 * 5 * 5, 4, 4) and G.dtype == np.float64
    assert G[0].tobytes() == C.tobytes()
    assert sum(np.allclose(g, C, atol=1e-12) for g in G) == 1  # (the centre is there once)
    assert pose_grid(C, 1.0, 0.5, 0.3, 2, z=0.5).shape[0] == 5 * 5 * 3 * 5
    assert pose_grid(C, 1.2, 0.5, 0.0, 0).shape[0] == 25 and pose_grid(C, 0.49, 0.5, 0.3, 1).shape[0] == 3


def test_zero_extents_give_the_centre_alone():
    C = centre(4)
    for args in ((0.0, 0.5, 0.0, 0), (0.0, 0.0, 0.0, 3), (1.0, 0.0, 0.3, 0), (0.2, 0.5, 0.0, 4)):
        G = pose_grid(C, *args)
        assert G.shape == (1, 4, 4) and G[0].tobytes() == C.tobytes(), args


def test_every_element_is_a_rigid_transform():
    G = pose_grid(centre(5), 1.5, 0.5, 0.4, 3, z=0.5)
    R = G[:, :3, :3]
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-12) and np.allclose(np.linalg.det(R), 1.0, atol=1e-12)
    assert np.array_equal(G[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (G.shape[0], 1)))


def test_order_and_frame():
    C = centre(6)
    step, half, ys = 0.5, np.deg2rad(30.0), 2
    G = pose_grid(C, 0.5, step, half, ys, z=0.5)
    D = np.linalg.inv(C) @ G  # the displacements in the centre's frame
    kz, ky, kx, kj = (a.ravel() for a in np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], [-2, -1, 0, 1, 2], indexing="ij"))
    keep = ~((kz == 0) & (ky == 0) & (kx == 0) & (kj == 0))
    want = np.stack([kx, ky, kz], axis=1)[keep] * step
    assert np.allclose(D[1:, :3, 3], want, atol=1e-12)  # ascending (dz, dy, dx, yaw), the yaw fastest, the centre taken out
    yaw = np.arctan2(D[1:, 1, 0], D[1:, 0, 0])
    assert np.allclose(yaw, kj[keep] * half / ys, atol=1e-12)
    assert np.allclose(D[1:, 2, :3], [0.0, 0.0, 1.0], atol=1e-12) and np.allclose(D[1:, :2, 2], 0.0, atol=1e-12)  # about the centre's z


def test_a_centre_that_is_no_matrix_is_refused():
    with pytest.raises(ValueError):
        pose_grid(np.eye(3), 1.0, 0.5, 0.1, 1)
