"""NumPy / Qhull restatement of the triangle-mesh distance of csrc/fbr_mesh.h.  It knows neither GJK nor the culling.

* a triangle against a solid hull: tests/hull_restatement.py on the triangle's three points against the hull's vertices (their Minkowski
  difference is a solid); negative where they intersect;
* a triangle against a triangle, closed form: if an edge of one pierces the other (segment against triangle) minus the depth of the
  deepest crossing -- the smaller of the end points' distances to the plane and the crossing point's distance to the triangle's sides --,
  else the smallest of the 9 segment-segment and the 6 point-triangle distances;
* a mesh distance: the plain double loop, the minimum of the signed values; the DISTANCE is that minimum clamped at 0 (``clamp``).  The
  signed value says how clear a verdict is: the tests keep their inputs out of the grey zone around 0."""
import numpy as np

import hull_restatement as hr

EPS = hr.EPS
_EDGES = ((0, 1), (1, 2), (2, 0))


def _dot(a, b):
    return np.einsum("ij,ij->i", a, b)


def point_triangle(p, a, b, c):
    """distance of the points p (N, 3) to the triangles a b c (N, 3) each; a zero-area triangle is its sides"""
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    size = np.maximum(np.maximum(_dot(b - a, b - a), _dot(c - a, c - a)), 1e-300)
    flat = nn <= 1e-24 * size * size
    nn1 = np.where(flat, 1.0, nn)
    h = _dot(p - a, n) / nn1
    foot = p - h[:, None] * n
    inside = ~flat
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= _dot(np.cross(v - u, foot - u), n) >= 0.0
    sides = np.minimum(np.minimum(hr._segment(p, a, b), hr._segment(p, b, c)), hr._segment(p, c, a))
    return np.where(inside, np.abs(h) * np.sqrt(nn1), sides)


def segment_segment(p1, q1, p2, q2):
    """distance of the segments p1 q1 and p2 q2 (N, 3): reached at an end point of one of them, or inside both where the lines come closest"""
    best = np.minimum(np.minimum(hr._segment(p1, p2, q2), hr._segment(q1, p2, q2)), np.minimum(hr._segment(p2, p1, q1), hr._segment(q2, p1, q1)))
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, b, c, f = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2), _dot(d1, r), _dot(d2, r)
    den = a * e - b * b
    ok = den > 1e-12 * a * e
    den1 = np.where(ok, den, 1.0)
    s, t = (b * f - c * e) / den1, (a * f - b * c) / den1
    mid = np.linalg.norm(r + s[:, None] * d1 - t[:, None] * d2, axis=1)
    ok &= (s >= 0.0) & (s <= 1.0) & (t >= 0.0) & (t <= 1.0)
    return np.where(ok, np.minimum(best, mid), best)


def pierce_depth(p, q, a, b, c):
    """(N,): > 0 where the segment p q crosses the inside of the triangle a b c, the depth of the crossing; else 0"""
    n = np.cross(b - a, c - a)
    ln = np.sqrt(np.maximum(_dot(n, n), 1e-300))
    dp, dq = _dot(p - a, n), _dot(q - a, n)
    cross = dp * dq < 0.0
    lam = np.where(cross, dp / np.where(cross, dp - dq, 1.0), 0.0)
    x = p + lam[:, None] * (q - p)
    inside = cross.copy()
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= _dot(np.cross(v - u, x - u), n) > 0.0
    rim = np.minimum(np.minimum(hr._segment(x, a, b), hr._segment(x, b, c)), hr._segment(x, c, a))
    depth = np.minimum(np.minimum(np.abs(dp), np.abs(dq)) / ln, rim)
    return np.where(inside, depth, 0.0)


def triangle_triangle(P, Q):
    """signed values (N,) of the triangles P, Q (N, 3, 3) in world coordinates"""
    depth = np.zeros(len(P))
    best = np.full(len(P), np.inf)
    for X, Y in ((P, Q), (Q, P)):
        for i, j in _EDGES:
            depth = np.maximum(depth, pierce_depth(X[:, i], X[:, j], Y[:, 0], Y[:, 1], Y[:, 2]))
        for i in range(3):
            best = np.minimum(best, point_triangle(X[:, i], Y[:, 0], Y[:, 1], Y[:, 2]))
    for i, j in _EDGES:
        for k, l in _EDGES:
            best = np.minimum(best, segment_segment(P[:, i], P[:, j], Q[:, k], Q[:, l]))
    return np.where(depth > 0.0, -depth, best)


def triangle_hull(tri, VB):
    """signed distance of the triangle tri (3, 3) and the solid hull of the points VB, both in world coordinates"""
    I, o = np.eye(3), np.zeros(3)
    return hr.hull_distance(I, o, tri, I, o, VB)


def world(R, c, X):
    return c + X @ R.T


def mesh_signed(RA, cA, trisA, VA, RB, cB, trisB, VB):
    """The minimum of the signed values over the triangles (pairs).  trisA / trisB (T, 3, 3) or None: that side is the solid hull of VA / VB
    (one side at least is a mesh).  Poses: R (3, 3), c (3,)."""
    if not (np.isfinite(RA).all() and np.isfinite(cA).all() and np.isfinite(RB).all() and np.isfinite(cB).all()):
        return np.nan
    if trisA is None:
        return mesh_signed(RB, cB, trisB, VB, RA, cA, None, VA)
    wa = world(RA, cA, np.asarray(trisA).reshape(-1, 3)).reshape(-1, 3, 3)
    if trisB is None:
        wb = world(RB, cB, VB)
        return min(triangle_hull(t, wb) for t in wa)
    wb = world(RB, cB, np.asarray(trisB).reshape(-1, 3)).reshape(-1, 3, 3)
    return float(triangle_triangle(np.repeat(wa, len(wb), axis=0), np.tile(wb, (len(wa), 1, 1))).min())


def clamp(signed):
    """the mesh DISTANCE of a signed value: exactly 0.0 where the two touch or intersect"""
    return np.where(np.isnan(signed), np.nan, np.maximum(signed, 0.0))


def pair_signed(R, c, hulls, meshes, pairs, rows=None):
    """(signed (S, P), scale (S, P)) of a hull set [(link, offset, rot, vertices)] with ``meshes`` {hull index: triangles}: pairs without a
    mesh get the signed hull distance of tests/hull_restatement.py.  ``rows``: the samples to evaluate (the others NaN)."""
    S, P = R.shape[0], len(pairs)
    diam = [float(np.linalg.norm(h[3][:, None] - h[3][None], axis=2).max()) for h in hulls]
    out, scale = np.full((S, P), np.nan), np.zeros((S, P))
    for k, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        scale[:, k] = hr.pair_scale(c[:, a], diam[a], c[:, b], diam[b])
        for s in (range(S) if rows is None else rows):
            if a in meshes or b in meshes:
                out[s, k] = mesh_signed(R[s, a], c[s, a], meshes.get(a), hulls[a][3], R[s, b], c[s, b], meshes.get(b), hulls[b][3])
            else:
                out[s, k] = hr.hull_distance(R[s, a], c[s, a], hulls[a][3], R[s, b], c[s, b], hulls[b][3])
    return out, scale


def pair_distances(signed, pairs, meshes):
    """the distances the device returns: mesh pairs clamped at 0, plain hull pairs signed"""
    out = signed.copy()
    for k, (a, b) in enumerate(pairs):
        if int(a) in meshes or int(b) in meshes:
            out[:, k] = clamp(signed[:, k])
    return out
