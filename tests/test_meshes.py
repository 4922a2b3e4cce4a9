"""Triangle-mesh collision distances off the GPU: the HIP-free text of csrc/fbr_mesh.h (g++, tests/emul/mesh_emul.cpp) against the restatement
of tests/mesh_restatement.py (which knows neither GJK nor the culling); the host side of flobaroid_amd/collision.py (Mesh, meshes from a
URDF, the collision set with fullMeshLinks and collisionMode "full"), the gradient refusals of flobaroid_amd/excitation.py with a stub
engine, and the C-ABI checks of fbr_model_set_hull_meshes.

Every comparison keeps out of the grey zone first: the restatement's signed value is a clear intersection or a clear gap, more than 100
bars from zero (a bar: 32 eps x the pair's scale |cB - cA| + diam hull A + diam hull B).  The assertion is the bar; intersections must come
back as exactly 0.0.  Culling on and off (a switch of the emulation only) must give the same bits everywhere.

Measured here (g++, -ffp-contract=off), in units of eps x scale: random soups of 1 .. 40 triangles against the shapes of
tests/hull_shapes.py 0.72 and against each other 1.08 (51 apart, 13 intersecting), the fixture meshes against each other 1.25 (12 apart, 8
intersecting), exact contacts at positive gaps 0 (the gap comes back exactly), the U-channel 0.040, the 100 cage placements 0.11; the
largest number of GJK iterations 9 (the cap FBR_HULL_MAX_ITER is 64; the tests hold it below a quarter).  The culling removed 91 % of the
triangle evaluations of the soups and 68 % of those of the fixture meshes ("Triangle meshes")."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hull_restatement as hr
import hull_shapes as hs
import mesh_restatement as mr
from common import GOLDEN, ROOT
from test_boxes import random_rotations
from test_hulls import _c, _p, tables

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "mesh_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libmesh_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_lib = None
EPS = np.finfo(np.float64).eps
MAX_ITER = 64  # FBR_HULL_MAX_ITER
BAR = 32.0     # x eps x scale
URDF = os.path.join(GOLDEN, "urdf")
TRIANGLES = {"Waist": 70, "LShp": 60, "LShr": 60, "LShy": 100, "LElb": 70, "LForearm": 70, "LWrMot2": 56, "LWrMot3": 70, "LSoftHandLink": 100}
WORST = {"iters": 0}


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC, os.path.join(ROOT, "include", "fbr.h")] + [os.path.join(_CSRC, h) for h in ("fbr_mesh.h", "fbr_hull.h", "fbr_box.h", "fbr_capsule.h",
                                                                                                   "fbr_math.h", "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


def mesh_tables(nhulls, meshes):
    """(mtab (H, 2) int32, tris (T, 9)) of {hull index: triangles}"""
    mtab, parts, n = np.zeros((nhulls, 2), dtype=np.int32), [], 0
    for h, t in meshes.items():
        t = np.asarray(t, dtype=np.float64).reshape(-1, 9)
        mtab[int(h)] = (n, len(t))
        parts.append(t)
        n += len(t)
    return mtab, _c(np.concatenate(parts) if parts else np.zeros((0, 9)))


def emul_pairs(fr, hulls, meshes, pairs, cull=True):
    """(dist (S, P), (evaluations, culled, most iterations)) of the frames fr (S, H, 12) from the library's own text on the CPU"""
    vbeg, v, fbeg, pl, ebeg, ed, diam = tables(hulls)
    mtab, tris = mesh_tables(len(hulls), meshes)
    fr, pr = _c(fr), _c(pairs, np.int32).reshape(-1, 2)
    S, P = fr.shape[0], len(pr)
    dist, stats = np.zeros((S, P)), np.zeros(3, dtype=np.int64)
    emul().mesh_pairs(ctypes.c_long(S), len(hulls), _p(fr), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), _p(diam), _p(mtab), _p(tris),
                      ctypes.c_long(len(tris)), P, _p(pr), int(cull), _p(dist), stats.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return dist, tuple(int(x) for x in stats)


def both(fr, hulls, meshes, pairs):
    """the emulation with the culling; asserted: the same bits without it, no evaluation near the iteration cap"""
    a, sa = emul_pairs(fr, hulls, meshes, pairs, True)
    b, sb = emul_pairs(fr, hulls, meshes, pairs, False)
    assert a.tobytes() == b.tobytes(), "culling changed a bit"
    assert sa[0] <= sb[0] and 4 * max(sa[2], sb[2]) < MAX_ITER  # (evaluations with the culling, without)
    WORST["iters"] = max(WORST["iters"], sa[2], sb[2])
    return a, sa, sb


def frames(R, c):
    """(S, H, 12) of R (S, H, 3, 3), c (S, H, 3)"""
    return np.concatenate([np.asarray(R).reshape(len(R), -1, 9), np.asarray(c).reshape(len(c), -1, 3)], axis=2)


def solid(link, tris, pad=0.5):
    """a Hull around the triangles: their points and the corners of their bounding box grown by ``pad`` (a single triangle has no hull)"""
    from flobaroid_amd.collision import Hull

    pts = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    lo, hi = pts.min(0) - pad, pts.max(0) + pad
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    return Hull(link, np.concatenate([pts, corners]), np.zeros(3))


def box_triangles(half, centre=(0.0, 0.0, 0.0)):
    """(12, 3, 3): the surface of a box"""
    v = hs.box(half) + np.asarray(centre)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([[v[a], v[b], v[c]] for a, b, c, d in quads] + [[v[a], v[c], v[d]] for a, b, c, d in quads])


def compare(A, triA, B, triB, RA, cA, RB, cB, why):
    """One pose of a pair (triX None: the solid hull): the grey-zone rule, then the emulation against the restatement.  Returns
    (deviation in eps x scale, signed restatement, emulation's value, evaluations with culling, without)"""
    signed = mr.mesh_signed(RA, cA, triA, A.vertices, RB, cB, triB, B.vertices)
    scale = hr.pair_scale(cA, A.diameter, cB, B.diameter)
    bar = BAR * EPS * scale
    assert abs(signed) > 100.0 * bar, (why, signed, "grey zone: change the input")
    meshes = {i: t for i, t in ((0, triA), (1, triB)) if t is not None}
    got, sa, sb = both(frames(np.stack([RA, RB])[None], np.stack([cA, cB])[None]), [A, B], meshes, [[0, 1]])
    got = float(got[0, 0])
    if signed < 0:
        assert got == 0.0, (why, signed, got)
        return 0.0, signed, got, sa[0], sb[0]
    assert abs(got - signed) <= bar, (why, signed, got)
    return abs(got - signed) / (EPS * scale), signed, got, sa[0], sb[0]


def _soup(rng, n, size):
    """(triangles (n, 3, 3), a Hull that holds them)"""
    c = rng.standard_normal((n, 1, 3)) * size
    t = c + rng.standard_normal((n, 3, 3)) * size * 0.5
    if n == 1 and rng.random() < 0.5:
        t[0, 2] = t[0, 1]  # (a zero-area triangle now and then)
    return t, solid("soup", t, pad=0.25 * size)


def test_soups_against_shapes_and_each_other():
    rng = np.random.default_rng(0)
    worst = {"shape": 0.0, "soup": 0.0}
    nsep = nhit = ev = ev0 = 0
    for i in range(64):
        nt = int(rng.integers(1, 41)) if i % 8 else (1, 40)[(i // 8) % 2]
        tri, A = _soup(rng, nt, rng.uniform(0.05, 0.3))
        if i % 2:
            B, triB, key = hs.zoo(rng, "shape", hs.KINDS[(i // 2) % len(hs.KINDS)]), None, "shape"
        else:
            triB, B = _soup(rng, int(rng.integers(1, 41)), rng.uniform(0.05, 0.3))
            key = "soup"
        RA, RB = random_rotations(rng, 2)
        cA = rng.standard_normal(3) * 0.3
        cB = cA + rng.standard_normal(3) * (0.6 if B.diameter < 2 else 4.0) * (0.5 if i % 4 < 2 else 1.0)
        if i % 16 == 5:  # the mesh as the second geometry: the roles swap
            dev, signed, got, a, b = compare(B, None, A, tri, RB, cB, RA, cA, (i, key))
        else:
            dev, signed, got, a, b = compare(A, tri, B, triB, RA, cA, RB, cB, (i, key))
        worst[key] = max(worst[key], dev)
        nsep, nhit, ev, ev0 = nsep + (signed > 0), nhit + (signed < 0), ev + a, ev0 + b
    print(f"soups, eps x scale: {worst}; {nsep} apart, {nhit} intersecting; the culling removed {1 - ev / ev0:.2%} of {ev0} evaluations; "
          f"most GJK iterations {WORST['iters']}")
    assert nsep >= 16 and nhit >= 8 and ev < ev0


def fixture_meshes():
    """{link: Mesh} of the nine left-arm links and the cage"""
    from flobaroid_amd.collision import meshes_from_urdf

    out = meshes_from_urdf(os.path.join(URDF, "walkman_left_arm.urdf"), list(TRIANGLES))
    out.update(meshes_from_urdf(os.path.join(URDF, "walkman_apriori.urdf"), ["TorsoProtections"]))
    return out


def test_fixture_meshes_against_each_other():
    rng = np.random.default_rng(1)
    ms = fixture_meshes()
    names = list(ms)
    worst, nsep, nhit, ev, ev0 = 0.0, 0, 0, 0, 0
    for i in range(20):
        a, b = rng.choice(len(names), 2, replace=False) if i else (names.index("LShy"), names.index("LSoftHandLink"))  # (100 x 100 first)
        A, B = ms[names[a]], ms[names[b]]
        RA, RB = random_rotations(rng, 2)
        cA = rng.standard_normal(3) * 0.3
        cB = cA + rng.standard_normal(3) * (0.08 if i % 2 else 0.3)
        dev, signed, got, x, y = compare(A.hull, A.triangles, B.hull, B.triangles, RA, cA, RB, cB, (names[a], names[b]))
        worst, nsep, nhit, ev, ev0 = max(worst, dev), nsep + (signed > 0), nhit + (signed < 0), ev + x, ev0 + y
    print(f"fixture meshes, eps x scale: {worst:.3g}; {nsep} apart, {nhit} intersecting; the culling removed {1 - ev / ev0:.2%} of {ev0} evaluations")
    assert nsep >= 5 and nhit >= 3


GAPS = (1e-3, 1e-9, 0.0, -1e-9, -1e-3)


def contact_kinds():
    """{kind: (triangles of A, f(gap) -> triangles of B)} on dyadic coordinates; a negative gap intersects"""
    up = lambda g: np.array([0.0, 0.0, g])  # noqa: E731
    flat = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    return {
        "vertex on face": (flat, lambda g: np.array([[0.25, 0.25, 0.0], [0.5, 0.25, 0.5], [0.25, 0.5, 0.5]]) + up(g)),
        "edge on edge": (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.0, -1.0]]),
                         lambda g: np.array([[0.5, -1.0, 0.0], [0.5, 1.0, 0.0], [0.5, 0.0, 1.0]]) + up(g)),
        "vertex on vertex": (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, -1.0], [0.0, 1.0, -1.0]]),
                             lambda g: np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]) + up(g)),
        # coplanar: B's vertex comes at A's side x = 0 within the plane; at a negative gap the two overlap
        "coplanar": (flat, lambda g: np.array([[-1.0, 0.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.25, 0.0]]) - np.array([g, 0.0, 0.0])),
        "zero area": (flat, lambda g: np.array([[0.25, 0.25, 0.0], [0.25, 0.25, 0.0], [0.5, 0.5, 1.0]]) + up(g)),
        "zero area in the plane": (flat, lambda g: np.array([[-1.0, 0.5, 0.0], [-1.0, 0.5, 0.0], [0.0, 0.25, 0.0]]) - np.array([g, 0.0, 0.0])),
    }


@pytest.mark.parametrize("kind", list(contact_kinds()))
def test_exact_contacts(kind):
    """each contact at five gaps, in three exact poses (as it is; both turned by pi / 2 about x and moved by a dyadic vector; A against
    the solid box below B's lowest vertex where the kind has one): positive gaps within the bar, zero and negative gaps exactly 0.0"""
    triA, fB = contact_kinds()[kind]
    worst = 0.0
    for R, c in ((np.eye(3), np.zeros(3)), (hs.TURNS["on_side"], np.array([0.5, -0.25, 2.0]))):
        for gap in GAPS:
            tA, tB = triA[None], fB(gap)[None]
            A, B = solid("a", tA), solid("b", tB)
            got, _, _ = both(frames(np.stack([R, R])[None], np.stack([c, c])[None]), [A, B], {0: tA, 1: tB}, [[0, 1]])
            got = float(got[0, 0])
            scale = hr.pair_scale(c, A.diameter, c, B.diameter)
            want = float(mr.clamp(mr.mesh_signed(R, c, tA, A.vertices, R, c, tB, B.vertices)))
            if gap > 0:
                assert abs(got - gap) <= BAR * EPS * scale and abs(want - gap) <= BAR * EPS * scale, (kind, gap, got, want)
                worst = max(worst, abs(got - gap) / (EPS * scale))
            else:
                assert got == 0.0, (kind, gap, got)
                assert want <= BAR * EPS * scale, (kind, gap, want)
            # the same through the swap: the mesh second, and identical triangles touch
            sw, _, _ = both(frames(np.stack([R, R])[None], np.stack([c, c])[None]), [B, A], {0: tB, 1: tA}, [[0, 1]])
            assert (abs(sw[0, 0] - gap) <= BAR * EPS * scale) if gap > 0 else sw[0, 0] == 0.0
    same, _, _ = both(frames(np.stack([np.eye(3)] * 2)[None], np.zeros((1, 2, 3))), [solid("a", triA[None])] * 2, {0: triA[None], 1: triA[None]}, [[0, 1]])
    assert same[0, 0] == 0.0
    print(f"{kind}: positive gaps within {worst:.3g} eps x scale")


def test_contacts_of_a_triangle_with_a_solid():
    """a triangle's vertex, edge and face on the top face of a box (a solid hull) at the five gaps: the facet pass is never entered, 0.0
    comes back where the hull routine returns a negative distance"""
    from flobaroid_amd.collision import Hull
    from test_hulls import emul_distance

    box = Hull("box", hs.box([0.5, 0.5, 0.25]), np.zeros(3))
    I, o = np.eye(3), np.zeros(3)
    kinds = {"vertex": np.array([[0.0, 0.0, 0.25], [0.25, 0.0, 0.75], [0.0, 0.25, 0.75]]),
             "edge": np.array([[-0.25, 0.0, 0.25], [0.25, 0.0, 0.25], [0.0, 0.0, 0.75]]),
             "face": np.array([[-0.25, -0.25, 0.25], [0.25, 0.0, 0.25], [0.0, 0.25, 0.25]])}
    for kind, t in kinds.items():
        for gap in GAPS:
            tri = (t + np.array([0.0, 0.0, gap]))[None]
            A = solid("t", tri)
            got, _, _ = both(frames(np.stack([I, I])[None], np.zeros((1, 2, 3))), [A, box], {0: tri}, [[0, 1]])
            sw, _, _ = both(frames(np.stack([I, I])[None], np.zeros((1, 2, 3))), [box, A], {1: tri}, [[0, 1]])
            scale = hr.pair_scale(o, A.diameter, o, box.diameter)
            signed = mr.mesh_signed(I, o, tri, A.vertices, I, o, None, box.vertices)
            assert abs(signed - gap) <= BAR * EPS * scale
            for g in (got[0, 0], sw[0, 0]):
                assert (abs(g - gap) <= BAR * EPS * scale) if gap > 0 else g == 0.0, (kind, gap, g)
    # deep inside the solid: 0.0, where the hull of the same triangle (made solid) is negative
    tri = (kinds["vertex"] - np.array([0.0, 0.0, 0.5]))[None] * 0.25
    A = solid("t", tri, pad=0.01)
    got, _, _ = both(frames(np.stack([I, I])[None], np.zeros((1, 2, 3))), [A, box], {0: tri}, [[0, 1]])
    assert got[0, 0] == 0.0 and emul_distance(A, box, I[None], o[None], I[None], o[None])[0][0] < -0.05


def test_a_mesh_vertex_outside_its_hull_within_the_tolerance_is_not_culled():
    """fbr_model_set_hull_meshes lets a triangle vertex lie 1e-9 x the diameter outside its hull's planes.  Mesh B has such a vertex at the
    farthest corner of its box hull, pushed out along the diagonal by 1.4e-9; two point-like triangles of A sit on the two diagonals, the
    first 0.25 - 0.6e-9 from the opposite, exact corner, the second 0.25 from the pushed corner's place: the second wins by 0.8e-9, and a
    sphere over the hull's vertices alone would put it at 0.25 and skip it.  The hull's sphere holds the mesh's vertices too: the same bits
    with and without the culling, and the value of the pushed vertex."""
    from flobaroid_amd.collision import Hull

    c, u = np.array([0.5, 0.5, 0.5]), np.ones(3) / np.sqrt(3.0)
    B = Hull("b", hs.box(c), np.zeros(3))
    out = 8e-10  # outside each of the three planes at the corner; the tolerance is 1e-9 x sqrt(3)
    triB = np.array([[-c, -c + [0.125, 0.0, 0.0], -c + [0.0, 0.125, 0.0]], [c + out, c - [0.125, 0.0, 0.0], c - [0.0, 0.125, 0.0]]])
    p0, p1 = -c - u * (0.25 - 0.6e-9), c + u * 0.25
    triA = np.array([[p0, p0, p0], [p1, p1, p1]])
    A = solid("a", triA)
    assert _validate([A, B], [0, 1], [[0, 1]], [(0, triA), (1, triB)]) == (0, "")
    assert _validate([A, B], [0, 1], [[0, 1]], [(0, triA), (1, triB + np.where(triB > 0.5, 2e-9, 0.0))])[0] == -1  # (twice as far: refused)
    I, o = np.eye(3), np.zeros(3)
    got, _, _ = both(frames(np.stack([I, I])[None], np.zeros((1, 2, 3))), [A, B], {0: triA, 1: triB}, [[0, 1]])
    want = 0.25 - out * np.sqrt(3.0)
    scale = hr.pair_scale(o, A.diameter, o, B.diameter)
    assert abs(got[0, 0] - want) <= BAR * EPS * scale and got[0, 0] < 0.25 - 1e-9
    assert abs(float(mr.mesh_signed(I, o, triA, A.vertices, I, o, triB, B.vertices)) - want) <= BAR * EPS * scale


def u_channel():
    """three slabs as one mesh: a floor |x| <= 0.5, |y| <= 1, -0.125 <= z <= 0 and two walls 0.125 thick and 0.5 high along y at x = -+0.5"""
    from flobaroid_amd.collision import Mesh

    tris = np.concatenate([box_triangles([0.5, 1.0, 0.0625], [0.0, 0.0, -0.0625]), box_triangles([0.0625, 1.0, 0.25], [-0.4375, 0.0, 0.25]),
                           box_triangles([0.0625, 1.0, 0.25], [0.4375, 0.0, 0.25])])
    return Mesh("channel", tris, np.zeros(3))


def test_u_channel_with_a_tetrahedron_in_it():
    from flobaroid_amd.collision import Hull
    from test_hulls import emul_distance

    ch = u_channel()
    tet = Hull("tetra", np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.0], [0.0, 0.125, 0.0], [0.0, 0.0, 0.125]]) - 0.03125, np.zeros(3))
    rng = np.random.default_rng(3)
    I, o = np.eye(3), np.zeros(3)
    worst, n = 0.0, 0
    for i in range(12):
        c = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.8, 0.8), rng.uniform(0.12, 0.4)])
        R = random_rotations(rng, 1)[0]
        dev, signed, got, _, _ = compare(ch.hull, ch.triangles, tet, None, I, o, R, c, ("channel", i))
        hull_d = hr.hull_distance(I, o, ch.hull.vertices, R, c, tet.vertices)
        assert emul_distance(ch.hull, tet, I[None], o[None], R[None], c[None])[0][0] < 0.0 and hull_d < -0.05 and got > 0.02
        worst, n = max(worst, dev), n + 1
    print(f"U-channel: {n} placements with a positive mesh distance inside the hull, {worst:.3g} eps x scale")


def cage_placements():
    """(cage Mesh, tetrahedron Hull, [(centre, signed mesh value, hull distance)]) of the grid of 2 cm tetrahedra in the cage's bounding box that
    lie more than 1 cm inside its hull and more than 1 cm from its triangles -- selected by the restatement"""
    from flobaroid_amd.collision import Hull

    cage = fixture_meshes()["TorsoProtections"]
    tet = Hull("tetra", np.array([[0.0, 0.0, 0.0], [0.02, 0.0, 0.0], [0.0, 0.02, 0.0], [0.0, 0.0, 0.02]]) - 0.005, np.zeros(3))
    lo, hi = cage.hull.bounds
    I, o = np.eye(3), np.zeros(3)
    sel = []
    for x in np.linspace(lo[0], hi[0], 7)[1:-1]:
        for y in np.linspace(lo[1], hi[1], 7)[1:-1]:
            for z in np.linspace(lo[2], hi[2], 7)[1:-1]:
                c = np.array([x, y, z])
                hd = hr.hull_distance(I, o, cage.hull.vertices, I, c, tet.vertices)
                if hd < -0.01:
                    md = mr.mesh_signed(I, o, cage.triangles, cage.hull.vertices, I, c, None, tet.vertices)
                    if md > 0.01:
                        sel.append((c, md, hd))
    return cage, tet, sel


def test_the_cage_is_mostly_empty_space():
    cage, tet, sel = cage_placements()
    assert len(sel) >= 1
    I, o = np.eye(3), np.zeros(3)
    worst = 0.0
    for c, md, hd in sel:
        dev, signed, got, _, _ = compare(cage.hull, cage.triangles, tet, None, I, o, I, c, ("cage", tuple(c)))
        assert got > 0.01 and hd < -0.01
        worst = max(worst, dev)
    print(f"cage: {len(sel)} of 125 placements have hull distance < -1 cm and mesh distance > 1 cm (deepest {min(h for _, _, h in sel):.3f} m, "
          f"largest mesh distance {max(m for _, m, _ in sel):.3f} m); {worst:.3g} eps x scale")


def test_iterations_stay_far_from_the_cap():
    """(runs after the comparisons above when the file runs in order; alone it checks one case)"""
    if WORST["iters"] == 0:
        test_u_channel_with_a_tetrahedron_in_it()
    print(f"most GJK iterations over the cases of this file: {WORST['iters']}")
    assert 0 < WORST["iters"] and 4 * WORST["iters"] < MAX_ITER


# ---- the host side ---------------------------------------------------------------------------------------------------------------------------
def test_meshes_from_urdf(tmp_path):
    from flobaroid_amd.collision import FBR_MAX_MESH_TRIANGLES, hulls_from_urdf, meshes_from_urdf, read_stl

    urdf = os.path.join(URDF, "walkman_left_arm.urdf")
    ms = meshes_from_urdf(urdf, list(TRIANGLES))
    hulls, _ = hulls_from_urdf(urdf, list(TRIANGLES))
    assert {n: len(m.triangles) for n, m in ms.items()} == TRIANGLES and list(ms) == list(TRIANGLES)
    for n, m in ms.items():
        assert m.link_name == n and np.array_equal(m.offset, hulls[n].offset)
        assert np.array_equal(m.hull.vertices, hulls[n].vertices) and np.array_equal(m.hull.planes, hulls[n].planes)
    cage = meshes_from_urdf(os.path.join(URDF, "walkman_apriori.urdf"), ["TorsoProtections"])["TorsoProtections"]
    raw = read_stl(os.path.join(URDF, "meshes", "walkman", "simple", "ProtectionSystem.STL"))
    assert len(cage.triangles) == 72 and len(np.unique(cage.triangles.reshape(-1, 3), axis=0)) == 48 and len(cage.hull.vertices) == 22
    assert np.array_equal(cage.triangles, raw * 0.001)  # the URDF scale
    assert FBR_MAX_MESH_TRIANGLES == 256 >= max(TRIANGLES.values())
    with pytest.raises(ValueError, match=r"LShy.*BottomUpperArm\.STL.*100"):
        meshes_from_urdf(urdf, ["LShy"], max_triangles=99)
    with pytest.raises(ValueError, match="nothing_there"):
        meshes_from_urdf(urdf, ["LShy", "nothing_there"])
    with pytest.raises(ValueError, match="DWYTorso"):  # in the URDF, but its STL file is not among the fixtures
        meshes_from_urdf(os.path.join(URDF, "walkman_apriori.urdf"), ["DWYTorso"])


@pytest.mark.parametrize("cfg", [{"fullMeshLinks": ["LSoftHandLink", "LForearm"], "worldCollisionMargin": 0.03}, {"collisionMode": "full"}])
def test_collision_set_with_meshes(cfg):
    from flobaroid_amd.collision import collision_set, world_hulls_from_urdf
    from test_hulls import left_arm_hulls

    topo, (hulls, _) = left_arm_hulls()
    ms = fixture_meshes()
    wh = world_hulls_from_urdf(os.path.join(URDF, "world_walkman_suspended.urdf"))
    plain = {k: v for k, v in cfg.items() if k not in ("fullMeshLinks", "collisionMode")}
    convex = collision_set(topo, {}, dict(plain, collisionMode="convex"), hulls=hulls, world_hulls=wh)
    cs = collision_set(topo, {}, cfg, hulls=hulls, world_hulls=wh, meshes=ms)
    assert cs["pair_names"] == convex["pair_names"] and np.array_equal(cs["columns"], convex["columns"])
    assert np.array_equal(cs["hull_pairs"], convex["hull_pairs"]) and np.array_equal(cs["margins"], convex["margins"])
    names = [h.link_name or h.name for h in cs["hulls"]]
    want = cfg.get("fullMeshLinks", [n for n in topo.link_names if n in ms])
    assert sorted(names[h] for h in cs["meshes"]) == sorted(want) and "TorsoProtections" not in names
    for h, t in cs["meshes"].items():
        assert np.array_equal(t, ms[names[h]].triangles) and np.array_equal(cs["hulls"][h].vertices, hulls[names[h]].vertices)
    # without meshes= the refusal is what it was; a link of fullMeshLinks without a mesh is named
    with pytest.raises(ValueError, match="need triangle meshes: not covered"):
        collision_set(topo, {}, cfg, hulls=hulls, world_hulls=wh)
    if "fullMeshLinks" in cfg:
        with pytest.raises(ValueError, match="LForearm"):
            collision_set(topo, {}, cfg, hulls=hulls, world_hulls=wh, meshes={"LSoftHandLink": ms["LSoftHandLink"]})


# ---- excitation: the set is accepted, its gradients are refused -------------------------------------------------------------------------------
class HostMeshEngine:
    """candidate_hull_distances from the restatement, meshes included: what excitation._collision_block needs of an Engine"""

    def __init__(self, topo, floating):
        self.topo, self.floating, self.n, self.calls = topo, floating, topo.num_dofs, []

    def set_hulls(self, hulls, pairs, offset_in_link_axes=False, meshes=None):
        from test_hulls import as_tuples

        self.hulls, self.pairs, self.mode, self.meshes = as_tuples(self.topo, hulls), np.asarray(pairs).reshape(-1, 2), offset_in_link_axes, dict(meshes or {})
        self.calls.append(("set_hulls", sorted(self.meshes)))

    def candidate_hull_distances(self, st, ncand, step=3, base_pos=None, device_out=None):
        S = st["q"].shape[0]
        T = S // ncand
        rows = [c * T + i for c in range(ncand) for i in range(0, T, step)]
        R, c = hr.hull_world(self.topo, self.hulls, st["q"], self.floating, st.get("rpy"), base_pos, self.mode)
        signed, _ = mr.pair_signed(R, c, self.hulls, self.meshes, self.pairs, rows)
        val, idx = hr.candidate_minimum(mr.pair_distances(signed, self.pairs, self.meshes), ncand, step)
        self.calls.append(("hull_distances", S, step))
        return {"dist": val, "idx": idx}


def block_configurations(q, config, rpy=None, bpos=None):
    """The configurations the reference's collision loop of ONE candidate visits, in its order: (q (N, n), rpy (N, 3) or None, bpos (N, 3)
    or None, tag (N,)) -- tag >= 0: the trajectory sample; < 0: minus the count of the transition configuration."""
    T = q.shape[0]
    rows = [(q[i], i, i) for i in range(0, T, int(config.get("collisionCheckStep", 3)))]  # (configuration, pose sample, tag)
    ns = int(config.get("transitionCollisionSamples", 10))
    if config.get("transitionDuration", 3.0) > 0 and ns > 0:
        if rpy is not None:
            poses = sorted(set(np.linspace(0, T - 1, 6).astype(int).tolist()) | {int(np.abs(rpy).sum(1).argmax())})
        else:
            poses = [0]
        count = 0
        for qb in (q[0], q[-1]):
            for j in range(ns):
                tau = (j + 1) / (ns + 1)
                s = 10 * tau**3 - 15 * tau**4 + 6 * tau**5
                for pz in poses:
                    count += 1
                    rows.append((s * qb, pz, -count))
    pz = [r[1] for r in rows]
    return (np.array([r[0] for r in rows]), None if rpy is None else rpy[pz], None if bpos is None else bpos[pz], np.array([r[2] for r in rows]))


def restate_mesh_block(topo, floating, cs, q, config, rpy=None, bpos=None, with_bar=False):
    """the reference's collision loop for ONE candidate, configuration by configuration, on the mesh restatement (restate_hull_block of
    tests/test_hulls.py with the pairs of a meshed hull served as meshes): (g (P,), {pair: the winning sample, or minus the count of the
    winning transition configuration}, {pair: the reference's argmin, which only a trajectory sample updates}).  ``with_bar``: also
    (bar (P,), deviation) -- the library's own text on the CPU (tests/emul) on the same configurations, its largest deviation from the
    restatement, and per pair the larger of 10 x that and 32 eps x the pair's scale at the winning configuration; asserted on the way: every
    configuration of a mesh pair is out of the grey zone (more than 100 bars from 0) and the emulation's minima lie within the bars."""
    from test_hulls import as_tuples, emul_eval

    hulls, P = as_tuples(topo, cs["hulls"]), len(cs["pair_names"])
    pairs = cs["hull_pairs"][cs["columns"][:, 1]]  # in the order of pair_names
    mode, meshes = bool(cs.get("offset_in_link_axes", False)), cs.get("meshes", {})
    Q, RPY, BP, tag = block_configurations(q, config, rpy, bpos)
    R, c = hr.hull_world(topo, hulls, Q, floating, RPY, BP, mode)
    signed, scale = mr.pair_signed(R, c, hulls, meshes, pairs)
    d = mr.pair_distances(signed, pairs, meshes) - cs["margins"]
    g, argmin, main, won = np.full(P, 1e10), {}, {}, np.zeros(P, dtype=np.int64)
    for r in range(len(Q)):
        for k in range(P):
            if d[r, k] < g[k]:
                g[k], argmin[k], won[k] = d[r, k], int(tag[r]), r
                if tag[r] >= 0:
                    main[k] = int(tag[r])
    if not with_bar:
        return g, argmin, main
    fr, _, _ = emul_eval(topo, floating, cs["hulls"], pairs, Q, RPY if floating else None, BP if floating else None, mode)
    emu, _, _ = both(fr, cs["hulls"], meshes, pairs)
    dev = float(np.abs(emu - cs["margins"] - d).max())
    bars = np.maximum(10.0 * dev, BAR * EPS * scale)
    mp = np.array([int(a) in meshes or int(b) in meshes for a, b in pairs])
    assert not ((np.abs(signed) <= 100.0 * bars) & mp[None, :]).any(), "a mesh pair in the grey zone: change the seed"
    e = emu - cs["margins"]
    # (the emulation's minimum, not its winner: a pair of two robot links has the same distance at every base pose of a transition
    # configuration, up to rounding, and which of those copies wins is a matter of the last bit)
    assert np.all(np.abs(e.min(axis=0) - g) <= bars[won, np.arange(P)])
    return g, argmin, main, bars[won, np.arange(P)], dev


def small_mesh_set(margin=0.02):
    """the gantry with the U-channel on its bed as a mesh and a tetrahedron on its carriage, a box on the column: [topo, collision set]"""
    from flobaroid_amd.collision import Hull, collision_set

    topo = hs.gantry()
    ch = u_channel()
    ch.link_name = ch.hull.link_name = "bed"
    hulls = {"bed": ch.hull, "column": Hull("column", hs.box([0.0625, 0.0625, 0.0625]), np.array([0.0, 1.5, 0.0])),
             "carriage": Hull("carriage", np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.0], [0.0, 0.125, 0.0], [0.0, 0.0, 0.125]]), np.array([-0.25, 0.0, -0.25]))}
    cfg = {"collisionMode": "convex", "fullMeshLinks": ["bed"], "worldCollisionMargin": margin}
    return topo, cfg, collision_set(topo, {}, cfg, hulls=hulls, meshes={"bed": ch})


def test_mesh_sets_in_the_collision_block_and_the_gradient_refusals():
    from flobaroid_amd import excitation as exc

    topo, cfg, cs = small_mesh_set()
    assert cs["pair_names"] == [("bed", "carriage")] and list(cs["meshes"]) == [0]
    C, T = 2, 8
    rng = np.random.default_rng(4)
    q = np.stack([rng.uniform(-0.1, 0.1, C * T), rng.uniform(-0.15, 0.15, C * T)], axis=1)  # the tetrahedron moves inside the channel
    st = {"q": q, "dq": np.zeros_like(q), "ddq": np.zeros_like(q)}
    config = dict(cfg, collisionCheckStep=3, transitionDuration=0.0)
    eng = HostMeshEngine(topo, False)
    coll = exc._collision_block(eng, st, C, config, cs)
    assert eng.calls[0] == ("set_hulls", [0]) and coll["g"].shape == (C, 1)
    assert np.all(coll["dist"] > 0.01), "inside the channel's hull, clear of its slabs"
    hull_only = HostMeshEngine(topo, False)
    hull_only.set_hulls(cs["hulls"], cs["hull_pairs"])
    assert np.all(hull_only.candidate_hull_distances(st, C, 3)["dist"] < 0.0)
    full = exc._collision_block(HostMeshEngine(topo, False), st, C, dict(config, collisionMode="full"), cs)
    assert np.array_equal(full["g"], coll["g"])
    trans = dict(config, transitionDuration=3.0, transitionCollisionSamples=2)
    blk = exc._collision_block(HostMeshEngine(topo, False), st, C, trans, cs)
    for c in range(C):
        g, argmin, main = restate_mesh_block(topo, False, cs, q[c * T:(c + 1) * T], trans)
        assert np.abs(blk["g"][c] - g).max() <= 1e-13 and blk["idx"][c, 0] == argmin.get(0, -1) and blk["argmin"][c, 0] == main.get(0, -1)
    # the configuration without a set that has meshes, and the gradient entry points
    plain = {k: v for k, v in cs.items() if k != "meshes"}
    for bad in (config, dict(config, collisionMode="full", fullMeshLinks=[])):
        with pytest.raises(ValueError, match="triangle"):
            exc._collision_block(eng, st, C, bad, plain)
    limits = {j: {"lower": -1.0, "upper": 1.0, "velocity": 1.0, "torque": 1.0} for j in topo.dof_names}
    for kw in ({}, {"hull_gradient": True}, {"box_gradient": True}):
        with pytest.raises(ValueError, match=r"triangle meshes.*bed"):
            exc.candidate_collision_gradient(eng, st, C, [], 50.0, config, cs, **kw)
        with pytest.raises(ValueError, match=r"triangle meshes.*bed"):
            exc.candidate_gradients_from_coefficients(eng, [], T, 50.0, None, None, limits, topo.dof_names, config, collision=cs, **kw)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_mesh_symbols_in_header_binding_and_library():
    from flobaroid_amd import _lib, collision

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    name = "fbr_model_set_hull_meshes"
    assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr)
    limits = {k: int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) for k in ("FBR_MAX_MESH_TRIANGLES", "FBR_MAX_MESH_PAIR_WORK")}
    assert limits == {"FBR_MAX_MESH_TRIANGLES": collision.FBR_MAX_MESH_TRIANGLES, "FBR_MAX_MESH_PAIR_WORK": collision.FBR_MAX_MESH_PAIR_WORK}
    assert limits["FBR_MAX_MESH_PAIR_WORK"] >= 170 * 160 and hasattr(_lib.Engine, "set_hull_meshes")
    assert lib.fbr_model_set_hull_meshes(None, 0, None, None, None) == -1  # FBR_E_INVALID: no model


def _validate(hulls, link, pairs, meshes, edit=None):
    """the checks of fbr_model_set_hull_meshes (the same text, tests/emul/mesh_emul.cpp): (0 or -1, message); meshes: [(hull, triangles)]"""
    _, _, fbeg, pl, _, _, diam = tables(hulls) if hulls else (None, None, _c([0], np.int32), np.zeros((0, 4)), None, None, np.zeros(0))
    arr = {"hull": _c([h for h, _ in meshes], np.int32), "tbeg": _c(np.cumsum([0] + [len(t) for _, t in meshes]), np.int32),
           "tris": _c(np.concatenate([np.asarray(t).reshape(-1, 9) for _, t in meshes]) if meshes else np.zeros((0, 9)))}
    if edit:
        edit(arr)
    link, pr = _c(link, np.int32), _c(pairs, np.int32).reshape(-1, 2)
    msg = ctypes.create_string_buffer(256)
    rc = emul().mesh_validate(len(hulls), _p(link), _p(fbeg), _p(pl), _p(diam), len(pr), _p(pr), len(meshes), _p(arr["hull"]), _p(arr["tbeg"]),
                              _p(arr["tris"]), msg, 256)
    return rc, msg.value.decode()


def test_set_hull_meshes_refuses_what_the_header_lists():
    rng = np.random.default_rng(6)
    soups = [_soup(rng, n, 0.2) for n in (5, 9, 3, 4)]
    hulls, tris = [h for _, h in soups], [t for t, _ in soups]
    link, pairs = [0, 2, 1, -1], [[0, 1], [0, 3], [1, 2]]
    ok = [(0, tris[0]), (1, tris[1])]
    assert _validate(hulls, link, pairs, ok) == (0, "") and _validate(hulls, link, pairs, []) == (0, "")
    assert _validate(hulls, link, pairs, [(1, tris[1]), (0, tris[0])]) == (0, "")  # any order

    def put(key, index, value):
        def edit(arr):
            arr[key].reshape(-1)[index] = value
        return edit

    big = np.tile(tris[0][:1], (257, 1, 1))
    a182 = np.tile(tris[0][:1], (182, 1, 1))
    b182 = np.tile(tris[1][:1], (182, 1, 1))
    bad = {
        "no hull set": dict(hulls=[], link=[], pairs=[], meshes=[]), "hull index": dict(meshes=[(4, tris[0])]), "negative index": dict(meshes=[(-1, tris[0])]),
        "given twice": dict(meshes=[(0, tris[0]), (0, tris[0])]), "world hull": dict(meshes=[(3, tris[3])]),
        "tbeg starts at 0": dict(meshes=ok, edit=put("tbeg", 0, 1)), "not ascending": dict(meshes=ok, edit=put("tbeg", 1, 99)),
        "no triangle": dict(meshes=[(0, tris[0]), (1, np.zeros((0, 3, 3)))]), "non-finite": dict(meshes=ok, edit=put("tris", 7, np.nan)),
        "outside face": dict(meshes=[(0, tris[0] * 3.0)]), "triangles,": dict(meshes=[(0, big)]),
        "triangle pairs": dict(meshes=[(0, a182), (1, b182)]),
    }
    for why, kw in bad.items():
        rc, msg = _validate(kw.get("hulls", hulls), kw.get("link", link), kw.get("pairs", pairs), kw["meshes"], kw.get("edit"))
        assert rc == -1 and msg, why
    for why in ("given twice", "world hull", "no triangle", "outside face", "triangle pairs"):
        kw = bad[why]
        assert why.split()[-1] in _validate(hulls, link, pairs, kw["meshes"], kw.get("edit"))[1], why
    assert "257 triangles" in _validate(hulls, link, pairs, bad["triangles,"]["meshes"])[1]
    # 182 x 182 is refused only for a pair of the set: with the pair (0, 1) gone the same meshes pass; 256 triangles pass
    assert _validate(hulls, link, [[0, 3], [1, 2]], bad["triangle pairs"]["meshes"]) == (0, "")
    assert _validate(hulls, link, pairs, [(0, big[:256])]) == (0, "")
