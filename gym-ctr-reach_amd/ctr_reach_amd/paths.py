"""Waypoint paths for CtrReachVecEnv.follow (a policy) and dls_ik_path (the DLS IK baseline): the
line, circle and helix paths the reference's src/ follows with both.

Every generator returns float64 numpy [M, K, 3]: K waypoints for each of M paths, in metres in the
robot's base frame.  Arguments broadcast over the paths: a point is [3] or [M, 3], a radius, pitch
or number of turns a scalar or [M].  The waypoints are closed forms of the path parameter
u_j = j / (K - 1), j = 0..K-1 (both ends included; K = 1: the single waypoint u = 1 of a line, the
end, and u = 0 of a circle or helix, the start).  No interpolation happens on the device: a denser
path is a larger K.
"""
import numpy as np

_AXES = {"x": (1, 2, 0), "y": (2, 0, 1), "z": (0, 1, 2)}     # axis -> (u, v, normal) coordinates


def _points(p):
    p = np.asarray(p, dtype=np.float64)
    if p.ndim == 1:
        p = p[None, :]
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("a point must be [3] or [M, 3]")
    return p


def _count(K):
    K = int(K)
    if K < 1:
        raise ValueError("a path needs at least one waypoint")
    return K


def line_path(start, end, K):
    """start + u_j (end - start): K evenly spaced waypoints from ``start`` to ``end``, both
    included (K = 1: ``end``)."""
    K = _count(K)
    a, b = np.broadcast_arrays(_points(start), _points(end))
    u = np.ones(1) if K == 1 else np.arange(K, dtype=np.float64) / (K - 1)
    out = a[:, None, :] + u[None, :, None] * (b - a)[:, None, :]
    out[:, -1, :] = b                          # the end itself, not start + 1.0 * (end - start)
    return out


def helix_path(centre, radius, pitch, turns, K, axis="z"):
    """``turns`` turns of radius ``radius`` around the line through ``centre`` along ``axis`` ("x",
    "y" or "z"), rising ``pitch`` metres per turn: with theta_j = 2 pi turns u_j and (u, v, w) the
    right-handed frame whose w is the axis,
        centre + radius (cos theta_j u + sin theta_j v) + pitch theta_j / (2 pi) w."""
    K = _count(K)
    if axis not in _AXES:
        raise ValueError("axis must be 'x', 'y' or 'z'")
    iu, iv, iw = _AXES[axis]
    c = _points(centre)
    r, p, n = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (radius, pitch, turns))
    m = max(c.shape[0], r.shape[0], p.shape[0], n.shape[0])
    c = np.broadcast_to(c, (m, 3))
    r, p, n = (np.broadcast_to(v, (m,)) for v in (r, p, n))
    u = np.zeros(1) if K == 1 else np.arange(K, dtype=np.float64) / (K - 1)
    rev = n[:, None] * u[None, :]              # revolutions so far, [M, K]
    theta = 2.0 * np.pi * rev
    out = np.repeat(c[:, None, :], K, axis=1).astype(np.float64)
    out[:, :, iu] += r[:, None] * np.cos(theta)
    out[:, :, iv] += r[:, None] * np.sin(theta)
    out[:, :, iw] += p[:, None] * rev
    return out


def circle_path(centre, radius, K, axis="z"):
    """One turn of radius ``radius`` around ``centre`` in the plane normal to ``axis``: a helix of
    pitch 0, closed (for K > 1 the last waypoint is the first one, bit for bit)."""
    out = helix_path(centre, radius, 0.0, 1.0, K, axis)
    out[:, -1, :] = out[:, 0, :]
    return out
