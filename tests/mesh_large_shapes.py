"""Meshes for the tests of fbr_model_set_large_hull_meshes (tests/test_meshes_large.py, tests/test_gpu_meshes_large.py), generated from seeds,
no files: sizes of a few decimetres, as the links of an arm.

* torus(): 20 x 16 quads = 640 triangles, concave (above FBR_MAX_MESH_TRIANGLES = 256);
* sphere(): a latitude-longitude sphere of 13 segments and 11 rings, 260 triangles on 132 vertices, all of them vertices of its hull: a mesh
  on a hull above FBR_MAX_HULL_VERTICES = 128 (a closed triangulated surface has F = 2 V - 4, so 260 triangles take 132 vertices);
* sheet(): a gently waved grid of 16 x 16 quads = 512 thin triangles, four times as long as wide: the worst case of a sphere tree;
* blob(seed): a sphere of 13 segments and 8 rings pushed in and out at random, 182 triangles: two of them make 182^2 = 33 124 triangle
  pairs, above FBR_MAX_MESH_PAIR_WORK = 32 768 with both meshes under 256;
* soup(seed, n): n random triangles -- n = L, L + 1, 2 L + 1 (L the leaf size: a root that is a leaf, the first split, a tree of two
  levels) and 257, the first count above the small cap.

hull_of(tris, link, pad): the flobaroid_amd.collision.Hull that carries a mesh -- pad None: the hull of its vertices; else of the vertices
and the corners of their bounding box grown by pad (eight vertices: a small hull)."""
import numpy as np


def _grid(P, wrap_u, wrap_v):
    """triangles (2 quads, 3, 3) of the point grid P (U, V, 3); wrap: the last row / column joins the first"""
    U, V = P.shape[:2]
    out = []
    for i in range(U if wrap_u else U - 1):
        for j in range(V if wrap_v else V - 1):
            a, b, c, d = P[i, j], P[(i + 1) % U, j], P[(i + 1) % U, (j + 1) % V], P[i, (j + 1) % V]
            out += [[a, b, c], [a, c, d]]
    return np.array(out)


def torus(R=0.2, r=0.07, nu=20, nv=16):
    u, v = np.meshgrid(2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv, indexing="ij")
    return _grid(np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=2), True, True)


def _latlong(nseg, nring, radius):
    """a closed sphere: nring - 1 rings of nseg points between two poles; 2 nseg (nring - 1) triangles; radius (nring + 1, nseg) or a number"""
    th = np.pi * np.arange(nring + 1) / nring
    ph = 2 * np.pi * np.arange(nseg) / nseg
    rad = np.broadcast_to(np.asarray(radius, dtype=np.float64), (nring + 1, nseg)).copy()
    rad[0], rad[-1] = rad[0, 0], rad[-1, 0]  # (one point a pole)
    P = rad[:, :, None] * np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None],
                                    np.broadcast_to(np.cos(th)[:, None], (nring + 1, nseg))], axis=2)
    P[0], P[-1] = [0.0, 0.0, rad[0, 0]], [0.0, 0.0, -rad[-1, 0]]  # (sin(pi) is not 0.0)
    out = []
    for i in range(nring):
        for j in range(nseg):
            a, b, c, d = P[i, j], P[i + 1, j], P[i + 1, (j + 1) % nseg], P[i, (j + 1) % nseg]
            if i > 0:
                out.append([a, c, d])
            if i < nring - 1:
                out.append([a, b, c])
    return np.array(out)


def sphere(radius=0.2):
    t = _latlong(13, 11, radius)
    assert len(t) == 260 and len(np.unique(t.reshape(-1, 3), axis=0)) == 132
    return t


def blob(seed, radius=0.15):
    rng = np.random.default_rng(seed)
    t = _latlong(13, 8, radius * (1.0 + 0.35 * rng.uniform(-1.0, 1.0, (9, 13))))
    assert len(t) == 182
    return t


def sheet(lx=0.8, ly=0.2, n=16, wave=0.02):
    x, y = np.meshgrid(lx * (np.arange(n + 1) / n - 0.5), ly * (np.arange(n + 1) / n - 0.5), indexing="ij")
    t = _grid(np.stack([x, y, wave * np.sin(7.0 * x) * np.cos(9.0 * y)], axis=2), False, False)
    assert len(t) == 512
    return t


def soup(seed, n, size=0.12):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 1, 3)) * size + rng.standard_normal((n, 3, 3)) * size * 0.5


def hull_of(tris, link, pad=0.05, offset=None):
    from flobaroid_amd.collision import Hull

    pts = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    if pad is not None:
        lo, hi = pts.min(0) - pad, pts.max(0) + pad
        pts = np.concatenate([pts, [[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]])
    return Hull(link, pts, np.zeros(3) if offset is None else np.asarray(offset, dtype=np.float64))
