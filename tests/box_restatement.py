"""An independent NumPy restatement of the oriented-box distance of csrc/fbr_box.h, vectorised over cases, in WORLD coordinates (the library
works in the frame of the first box), and the two yardsticks it is held against:

* ``qp_distance`` -- separated boxes: min |x - y| over x in A, y in B as a box-constrained least-squares problem in the six box
  coordinates, solved by enumerating all 3^6 active sets;
* ``hull_depth`` -- overlapping boxes: the smallest facet offset of the convex hull of the 64 vertices of the Minkowski difference B - A
  (scipy.spatial.ConvexHull), i.e. the minimum translation that separates them.

Link poses come from tests/np_dynamics.world_kinematics: no code shared with the kernels."""
import itertools

import numpy as np

from capsule_restatement import candidate_minimum  # noqa: F401  (the minimum rules are the capsules')
from np_dynamics import rpy_R, world_kinematics

PARALLEL = 1e-12
SIGNS = np.array(list(itertools.product((-1.0, 1.0), repeat=3)))  # (8, 3)


def _dot(u, v):
    return (u * v).sum(-1)


def sat_axes(RA, RB):
    """(axes (N, 15, 3) normalised, len2 (N, 9) squared lengths of the cross products, used (N, 15))"""
    a = np.swapaxes(RA, -1, -2)  # rows: the axes of A
    b = np.swapaxes(RB, -1, -2)
    cr = np.cross(a[:, :, None, :], b[:, None, :, :]).reshape(-1, 9, 3)
    len2 = _dot(cr, cr)
    used = len2 >= PARALLEL
    with np.errstate(invalid="ignore", divide="ignore"):
        crn = cr / np.sqrt(len2)[..., None]
    axes = np.concatenate([a, b, np.where(used[..., None], crn, 0.0)], axis=1)
    return axes, len2, np.concatenate([np.ones((len(RA), 6), dtype=bool), used], axis=1)


def sat_gap(RA, cA, hA, RB, cB, hB):
    """max over the 15 axes of |ax . (cB - cA)| - r_A(ax) - r_B(ax), the radii from the dot products with every box axis"""
    axes, _, used = sat_axes(RA, RB)
    d = (cB - cA)[:, None, :]
    rA = (np.abs(np.einsum("nkx,nxi->nki", axes, RA)) * hA[:, None, :]).sum(-1)
    rB = (np.abs(np.einsum("nkx,nxi->nki", axes, RB)) * hB[:, None, :]).sum(-1)
    g = np.abs(_dot(axes, d)) - rA - rB
    return np.where(used, g, -np.inf).max(axis=1)


def _vertices(R, c, h):
    """the 8 corners (N, 8, 3)"""
    return c[:, None, :] + np.einsum("nxi,nvi->nvx", R, SIGNS[None] * h[:, None, :])


def _point_box(pts, R, c, h):
    """squared distance of points (N, V, 3) to the solid box"""
    loc = np.einsum("nvx,nxi->nvi", pts - c[:, None, :], R)
    e = np.maximum(np.abs(loc) - h[:, None, :], 0.0)
    return _dot(e, e)


def _edges(R, c, h):
    """(origins (N, 12, 3), directions (N, 12, 3)): 4 edges along each axis, from the low to the high end"""
    o, d = [], []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        for sj in (-1.0, 1.0):
            for sk in (-1.0, 1.0):
                loc = np.zeros((len(R), 3))
                loc[:, i], loc[:, j], loc[:, k] = -h[:, i], sj * h[:, j], sk * h[:, k]
                o.append(c + np.einsum("nxi,ni->nx", R, loc))
                d.append(2.0 * h[:, i, None] * R[:, :, i])
    return np.stack(o, axis=1), np.stack(d, axis=1)


def _segments(o1, d1, o2, d2):
    """squared distance of segments, broadcast; clamping as in Ericson 5.1.9 without thresholds except: a e - b^2 <= 1e-12 a e takes s = 0"""
    r = o1 - o2
    a, e, b, c, f = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2), _dot(d1, r), _dot(d2, r)
    den = a * e - b * b
    ok = den > PARALLEL * a * e
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(ok, np.clip((b * f - c * e) / np.where(ok, den, 1.0), 0.0, 1.0), 0.0)
        t = (b * s + f) / e
        s = np.where(t < 0.0, np.clip(-c / a, 0.0, 1.0), np.where(t > 1.0, np.clip((b - c) / a, 0.0, 1.0), s))
        t = np.clip(t, 0.0, 1.0)
    v = r + s[..., None] * d1 - t[..., None] * d2
    return _dot(v, v)


def separated_distance(RA, cA, hA, RB, cB, hB):
    """the exact distance by feature enumeration (meaningful where the boxes are separated)"""
    vA, vB = _vertices(RA, cA, hA), _vertices(RB, cB, hB)
    best = np.minimum(_point_box(vB, RA, cA, hA).min(1), _point_box(vA, RB, cB, hB).min(1))
    oA, dA = _edges(RA, cA, hA)
    oB, dB = _edges(RB, cB, hB)
    ee = _segments(oA[:, :, None, :], dA[:, :, None, :], oB[:, None, :, :], dB[:, None, :, :])
    return np.sqrt(np.minimum(best, ee.reshape(len(RA), -1).min(1)))


def box_distance(RA, cA, hA, RB, cB, hB):
    """signed distance (N,) of N box pairs: the SAT gap where it is <= 0, else the exact distance; NaN where an input is not finite"""
    RA, cA, hA, RB, cB, hB = (np.asarray(x, dtype=np.float64) for x in (RA, cA, hA, RB, cB, hB))
    bad = ~(np.isfinite(RA).all((1, 2)) & np.isfinite(RB).all((1, 2)) & np.isfinite(cA).all(1) & np.isfinite(cB).all(1))
    z = lambda x: np.where(bad.reshape((-1,) + (1,) * (x.ndim - 1)), 0.0, x)  # noqa: E731
    RA, cA, RB, cB = z(RA), z(cA), z(RB), z(cB)
    gap = sat_gap(RA, cA, hA, RB, cB, hB)
    out = gap.copy()
    sep = gap > 0.0
    if sep.any():
        out[sep] = separated_distance(RA[sep], cA[sep], hA[sep], RB[sep], cB[sep], hB[sep])
    out[bad] = np.nan
    return out


def pair_scale(cA, hA, cB, hB):
    return np.linalg.norm(cB - cA, axis=-1) + np.linalg.norm(hA, axis=-1) + np.linalg.norm(hB, axis=-1)


# ---- yardsticks ------------------------------------------------------------------------------------------------------------------------
def qp_distance(RA, cA, hA, RB, cB, hB):
    """min |d + M z| over |z| <= (hA, hB), M = [-RA, RB], d = cB - cA: every active set (each coordinate at its lower bound, at its upper
    bound, or free), the free coordinates by least squares, the smallest value among the feasible candidates"""
    N = len(RA)
    M = np.concatenate([-RA, RB], axis=2)  # (N, 3, 6)
    bound = np.concatenate([hA, hB], axis=1)
    d = cB - cA
    best = np.full(N, np.inf)
    for state in itertools.product((-1, 0, 1), repeat=6):
        st = np.array(state)
        free = st == 0
        z = bound * st
        res = d + np.einsum("nxi,ni->nx", M, z)
        if free.any():
            MF = M[:, :, free]
            zf = -np.einsum("nix,nx->ni", np.linalg.pinv(MF), res)
            feas = (np.abs(zf) <= bound[:, free] * (1 + 1e-12)).all(1)
            res = res + np.einsum("nxi,ni->nx", MF, zf)
        else:
            feas = np.ones(N, dtype=bool)
        val = np.linalg.norm(res, axis=1)
        best = np.where(feas & (val < best), val, best)
    return best


def hull_depth(RA, cA, hA, RB, cB, hB):
    """overlapping boxes, one case: minus the distance from the origin to the nearest facet of hull(B - A) (<= 0 when they overlap)"""
    from scipy.spatial import ConvexHull

    vA = _vertices(RA[None], cA[None], hA[None])[0]
    vB = _vertices(RB[None], cB[None], hB[None])[0]
    pts = (vB[:, None, :] - vA[None, :, :]).reshape(-1, 3)
    eq = ConvexHull(pts).equations  # n . x + off <= 0 inside, |n| = 1
    return float(eq[:, 3].max())


# ---- boxes on robots --------------------------------------------------------------------------------------------------------------------
def link_poses(topo, q, floating=False, rpy=None, base_pos=None):
    """(R [L] of (S, 3, 3), p [L] of (S, 3)) at joint positions q (S, n): world_T_base = (RPY(rpy)^T, base_pos) with a floating base"""
    q = np.asarray(q, dtype=np.float64)
    S = q.shape[0]
    z = np.zeros((S, 3))
    if floating and rpy is not None:
        R = np.transpose(rpy_R(np.asarray(rpy, dtype=np.float64)), (0, 2, 1))
        pb = z if base_pos is None else np.asarray(base_pos, dtype=np.float64)
    else:
        R, pb = np.tile(np.eye(3), (S, 1, 1)), z
    k = world_kinematics(topo, q, 0 * q, 0 * q, R, z, z, z, z, p_b=pb)
    return k["R"], k["p"]


def box_world(topo, boxes, q, floating=False, rpy=None, base_pos=None, center_in_link_axes=False):
    """(R (S, nb, 3, 3), c (S, nb, 3), h (nb, 3)) of ``boxes`` [(link index or -1, half, centre, rot or None)]"""
    Rl, pl = link_poses(topo, q, floating, rpy, base_pos)
    S = np.asarray(q).shape[0]
    R, c = np.empty((S, len(boxes), 3, 3)), np.empty((S, len(boxes), 3))
    for i, (l, h, cen, rot) in enumerate(boxes):
        cen = np.asarray(cen, dtype=np.float64)
        if l < 0:
            R[:, i], c[:, i] = np.asarray(rot, dtype=np.float64), cen
        else:
            R[:, i] = Rl[l]
            c[:, i] = pl[l] + (np.einsum("sij,j->si", Rl[l], cen) if center_in_link_axes else cen)
    return R, c, np.array([b[1] for b in boxes], dtype=np.float64).reshape(-1, 3)


def pair_distances(R, c, h, pairs):
    """(dist (S, P), scale (S, P)) of the box pairs at every sample"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    S, P = R.shape[0], len(pairs)
    ia, ib = pairs[:, 0], pairs[:, 1]
    f = lambda x: x.reshape((S * P,) + x.shape[2:])  # noqa: E731
    hA, hB = np.broadcast_to(h[ia], (S, P, 3)), np.broadcast_to(h[ib], (S, P, 3))
    d = box_distance(f(R[:, ia]), f(c[:, ia]), f(hA), f(R[:, ib]), f(c[:, ib]), f(hB)).reshape(S, P)
    return d, pair_scale(c[:, ia], hA, c[:, ib], hB)
