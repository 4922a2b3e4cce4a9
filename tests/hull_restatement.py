"""NumPy / Qhull restatement of the signed distance of two convex polytopes, independent of GJK and of the facet pass of csrc/fbr_hull.h:
the V_A V_B vertices of the Minkowski difference A - B are formed in world coordinates and handed to Qhull.  The origin inside: the largest
facet offset (<= 0, minus the minimum translation that separates the two); otherwise the smallest point-to-triangle distance over the facets.
Also the world poses of a hull set (link poses from tests/box_restatement.py) and the per-candidate minimum."""
import numpy as np
from scipy.spatial import ConvexHull

import box_restatement as br

EPS = np.finfo(np.float64).eps


def _segment(p, a, b):
    """distance of the points p (N, 3) to the segments a -- b (N, 3)"""
    ab = b - a
    t = np.clip(np.einsum("ij,ij->i", p - a, ab) / np.maximum(np.einsum("ij,ij->i", ab, ab), 1e-300), 0.0, 1.0)
    return np.linalg.norm(p - (a + t[:, None] * ab), axis=1)


def origin_to_triangles(a, b, c):
    """distance of the origin to the triangles (N, 3) x 3: the distance to the plane where the foot lies inside, else to the nearest side"""
    n = np.cross(b - a, c - a)
    nn = np.maximum(np.einsum("ij,ij->i", n, n), 1e-300)
    h = np.einsum("ij,ij->i", a, n) / nn          # the foot of the origin: h n
    foot = h[:, None] * n
    inside = np.ones(len(a), dtype=bool)
    for p, q in ((a, b), (b, c), (c, a)):
        inside &= np.einsum("ij,ij->i", np.cross(q - p, foot - p), n) >= 0.0
    o = np.zeros_like(a)
    sides = np.minimum(np.minimum(_segment(o, a, b), _segment(o, b, c)), _segment(o, c, a))
    return np.where(inside, np.abs(h) * np.sqrt(nn), sides)


def hull_distance(RA, cA, VA, RB, cB, VB):
    """signed distance of the hulls with vertices VA (in the axes RA at cA) and VB (RB at cB)"""
    if not (np.isfinite(RA).all() and np.isfinite(cA).all() and np.isfinite(RB).all() and np.isfinite(cB).all()):
        return np.nan
    wa, wb = cA + VA @ RA.T, cB + VB @ RB.T
    diff = (wa[:, None, :] - wb[None, :, :]).reshape(-1, 3)
    qh = ConvexHull(diff)
    off = qh.equations[:, 3] / np.linalg.norm(qh.equations[:, :3], axis=1)
    if off.max() <= 0.0:
        return float(off.max())
    tri = qh.points[qh.simplices]
    return float(origin_to_triangles(tri[:, 0], tri[:, 1], tri[:, 2]).min())


def pair_scale(cA, dA, cB, dB):
    return np.linalg.norm(np.asarray(cB) - np.asarray(cA), axis=-1) + dA + dB


def hull_world(topo, hulls, q, floating=False, rpy=None, base_pos=None, offset_in_link_axes=False):
    """(R (S, H, 3, 3), c (S, H, 3)) of the hulls [(link or -1, offset, rot or None, vertices)]"""
    boxes = [(h[0], np.ones(3), h[1], h[2]) for h in hulls]
    R, c, _ = br.box_world(topo, boxes, q, floating, rpy, base_pos, offset_in_link_axes)
    return R, c


def pair_distances(R, c, hulls, pairs, rows=None):
    """(dist (S, P), scale (S, P)); ``rows``: the samples to evaluate (the others NaN)"""
    S, P = R.shape[0], len(pairs)
    diam = [float(np.linalg.norm(h[3][:, None] - h[3][None], axis=2).max()) for h in hulls]
    dist = np.full((S, P), np.nan)
    scale = np.zeros((S, P))
    for k, (a, b) in enumerate(pairs):
        scale[:, k] = pair_scale(c[:, a], diam[a], c[:, b], diam[b])
        for s in (range(S) if rows is None else rows):
            dist[s, k] = hull_distance(R[s, a], c[s, a], hulls[a][3], R[s, b], c[s, b], hulls[b][3])
    return dist, scale


candidate_minimum = br.candidate_minimum
