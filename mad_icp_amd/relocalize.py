"""Pose hypotheses for Pipeline.mapScorePoses / Pipeline.mapRelocalize: a grid of positions times a fan of yaws around a pose.
Plain numpy, nothing of the device."""
import numpy as np


def _steps(half_extent, step):
    """the multiples i of `step` with |i step| <= half_extent, as integers -m .. m (m = 0 when either is not positive)"""
    if not (half_extent > 0.0 and step > 0.0):
        return np.zeros(1, np.int64)
    m = int(np.floor(half_extent / step + 1e-9))
    return np.arange(-m, m + 1, dtype=np.int64)


def pose_grid(center, xy_half_extent, xy_step, yaw_half_extent, yaw_steps, z=0):
    """(K, 4, 4) float64 hypotheses around `center` (4, 4): center @ translate(dx, dy, dz) @ rotate_z(yaw) — the translation is in
    the centre's frame, the yaw about its z axis behind it.

    dx, dy  the multiples of xy_step within [-xy_half_extent, xy_half_extent]
    dz      the multiples of xy_step within [-z, z] (z = 0: a planar grid)
    yaw     j * yaw_half_extent / yaw_steps for j = -yaw_steps .. yaw_steps (radians; yaw_steps = 0 or yaw_half_extent = 0: no fan)

    Order: element 0 is the centre itself, always; behind it every other combination in ascending (dz, dy, dx, yaw) order, the
    yaw running fastest.  K = (2 mx + 1)^2 (2 mz + 1) (2 yaw_steps + 1); zero extents give K = 1."""
    C = np.asarray(center, np.float64)
    if C.shape != (4, 4):
        raise ValueError("center must be (4, 4)")
    ixy = _steps(float(xy_half_extent), float(xy_step))
    iz = _steps(float(z), float(xy_step))
    jy = np.arange(-int(yaw_steps), int(yaw_steps) + 1, dtype=np.int64) if (int(yaw_steps) > 0 and yaw_half_extent > 0.0) else np.zeros(1, np.int64)
    kz, ky, kx, kj = (a.ravel() for a in np.meshgrid(iz, ixy, ixy, jy, indexing="ij"))
    here = (kz == 0) & (ky == 0) & (kx == 0) & (kj == 0)
    order = np.concatenate([np.flatnonzero(here), np.flatnonzero(~here)])  # (the centre first, the rest as they stand)
    kz, ky, kx, kj = kz[order], ky[order], kx[order], kj[order]
    yaw = kj * (float(yaw_half_extent) / max(int(yaw_steps), 1))
    D = np.tile(np.eye(4), (order.size, 1, 1))
    D[:, 0, 0] = D[:, 1, 1] = np.cos(yaw)
    D[:, 1, 0] = np.sin(yaw)
    D[:, 0, 1] = -D[:, 1, 0]
    D[:, 0, 3] = kx * float(xy_step)
    D[:, 1, 3] = ky * float(xy_step)
    D[:, 2, 3] = kz * float(xy_step)
    out = C[None] @ D
    out[0] = C  # (the centre itself, not centre times an identity)
    return out
