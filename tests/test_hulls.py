"""Convex-hull collision distances off the GPU: the HIP-free text of csrc/fbr_hull.h (g++, tests/emul/hull_emul.cpp) against the Qhull
restatement of tests/hull_restatement.py (which knows neither GJK nor the facet pass) and, on boxes, against tests/box_restatement.py; the
host side of flobaroid_amd/collision.py (STL reader, Hull tables, hulls from a URDF, the collision set), the collision block of
flobaroid_amd/excitation.py with a stub engine, and the C-ABI.

Measured here (g++ 11, -ffp-contract=off), in units of eps x the pair's scale |cB - cA| + diam A + diam B: random clouds of 4 .. 40 points
1.6, scaled to touch (1e-7 apart, 1e-3 deep) 0.24, a tetrahedron against a large hull 0.53, boxes as hulls against the box restatement 2.2; the
largest number of GJK iterations 7, a ninth of the cap (FBR_HULL_MAX_ITER 64).  The bar of every comparison is the larger of 10 x the
deviation measured on the same inputs and 32 eps x scale ("Convex-hull collision distances").

The shapes of tests/hull_shapes.py (the vertex cap of 128, a 64-gon prism, a sphere, a cone whose apex joins 127 faces, a tetrahedron,
1 mm and 10 m), same units: all 64 ordered pairs of the eight kinds in 12 random poses each 3.46 (the 10 m slab against the cone; 465
separated, 303 touching or overlapping), 18 iterations at most; flat bottoms on flat tops with exactly parallel faces at five gaps,
600 cases, 0.00064 (dyadic sizes: next to nothing is rounded), 6 iterations; edge on edge, apex on face, apex on apex, edge on face and a
prism's side edge on a prism's cap from 1e-2 apart to 1e-3 deep 2.27 (apex on apex, touching), 6 iterations.  World coordinates of
these cases stay within the pair's scale: the restatement rounds them, so that a 1 mm pair placed 0.3 m from the origin measured the
restatement's 33 eps x scale, not the routine's.  Four edits of a scratch copy of csrc/fbr_hull.h were each caught by these tests: the
facet pass without its edge pairs (zoo pairs, contact kinds), the support key (ia << 6) | ib (zoo pairs, parallel stacking), a cap of 8
iterations (zoo pairs), GJK without its |v|^2 <= floor test (parallel stacking and contact kinds: the facet pass does not run)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import box_restatement as br
import hull_restatement as hr
import hull_shapes as hs
from common import GOLDEN, ROOT, load_topo, random_states
from test_boxes import all_cases, random_rotations

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "hull_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libhull_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lib = None
EPS = np.finfo(np.float64).eps
MAX_ITER = 64  # FBR_HULL_MAX_ITER
URDF = os.path.join(GOLDEN, "urdf")
MESHES = {"BottomUpperArm": 52, "Elbow": 37, "Forearm": 36, "ForearmPitch": 30, "ForearmRoll": 37, "ShoulderPitch": 32, "SoftHandOpen": 52,
          "TopUpperArm": 32, "Waist": 37}


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC, os.path.join(ROOT, "include", "fbr.h")] + [os.path.join(_CSRC, h) for h in ("fbr_hull.h", "fbr_box.h", "fbr_capsule.h", "fbr_math.h",
                                                                                                   "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


def _c(a, t=np.float64):
    return np.ascontiguousarray(a, dtype=t)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp if a.dtype == np.float64 else _ip)


def tables(hulls):
    """(vbeg, verts, fbeg, planes, ebeg, edges, diam) of a list of Hull objects, as fbr_model_set_hulls takes them"""
    beg = lambda parts: _c(np.cumsum([0] + [len(x) for x in parts]), np.int32)  # noqa: E731
    V, F, E = [h.vertices for h in hulls], [h.planes for h in hulls], [h.edges for h in hulls]
    return (beg(V), _c(np.concatenate(V)), beg(F), _c(np.concatenate(F)), beg(E), _c(np.concatenate(E), np.int32), _c([h.diameter for h in hulls]))


def emul_distance(A, B, RA, cA, RB, cB):
    """(dist (N,), GJK iterations (N,), facet pass entered (N,)) of N poses of the hulls A and B"""
    vbeg, v, fbeg, pl, ebeg, ed, diam = tables([A, B])
    RA, cA, RB, cB = (_c(x) for x in (RA, cA, RB, cB))
    N = len(RA)
    out, it = np.zeros(N), np.zeros(N, dtype=np.int32)
    emul().hull_distance(ctypes.c_long(N), _p(RA), _p(cA), _p(RB), _p(cB), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), _p(diam), _p(out), _p(it))
    return out, it % 1000, it >= 1000


def link_index(topo, hulls):
    names = list(topo.link_names)
    return [-1 if h.link_name is None else names.index(h.link_name) for h in hulls]


def as_tuples(topo, hulls):
    """[(link or -1, offset, rot or None, vertices)]: what tests/hull_restatement.py takes"""
    return [(l, h.offset, h.rot, h.vertices) for l, h in zip(link_index(topo, hulls), hulls)]


def emul_eval(topo, floating, hulls, pairs, q, rpy=None, base_pos=None, offset_in_link_axes=False):
    """(frames (S, H, 12), dist (S, P), iterations (S, P)) from the library's own lane walk and hull routine on the CPU"""
    parent, dof, jt = _c(topo.parent, np.int32), _c(topo.dof_index, np.int32), _c(topo.joint_type, np.int32)
    rR, rp, ax = _c(topo.rest_R).reshape(-1), _c(topo.rest_p).reshape(-1), _c(topo.axis).reshape(-1)
    link = _c(link_index(topo, hulls), np.int32)
    off = _c([h.offset for h in hulls]).reshape(-1)
    rot = _c([np.eye(3) if h.rot is None else h.rot for h in hulls]).reshape(-1)
    vbeg, v, fbeg, pl, ebeg, ed, _ = tables(hulls)
    pr = _c(pairs, np.int32).reshape(-1)
    q = _c(q)
    S, P = q.shape[0], pr.size // 2
    rpy = None if rpy is None else _c(rpy)
    bp = None if base_pos is None else _c(base_pos)
    fr, dist, it = np.zeros((S, len(hulls), 12)), np.zeros((S, P)), np.zeros((S, P), dtype=np.int32)
    rc = emul().hull_eval(topo.num_links, topo.num_dofs, _p(parent), _p(dof), _p(rR), _p(rp), _p(ax), _p(jt), int(floating), len(hulls), _p(link), _p(off),
                          _p(rot), int(offset_in_link_axes), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), P, _p(pr), ctypes.c_long(S), _p(q),
                          _p(rpy), _p(bp), _p(fr), _p(dist), _p(it))
    assert rc == 0
    return fr, dist, it


# ---- the emulation against the restatement ---------------------------------------------------------------------------------------------------
def _cloud(rng, n, size):
    from flobaroid_amd.collision import Hull

    return Hull("cloud", rng.standard_normal((n, 3)) * size, np.zeros(3))


def _deviation(A, B, RA, cA, RB, cB):
    """(|emulation - restatement| / (eps scale), restatement, iterations, facet pass) of one pose"""
    want = hr.hull_distance(RA, cA, A.vertices, RB, cB, B.vertices)
    got, it, facet = emul_distance(A, B, RA[None], cA[None], RB[None], cB[None])
    return abs(got[0] - want) / (EPS * hr.pair_scale(cA, A.diameter, cB, B.diameter)), want, int(it[0]), bool(facet[0])


def test_emulation_equals_the_restatement_on_random_hulls():
    """random clouds of 4 .. 40 points in random poses; each pair also moved along the line of centres until it is 1e-7 apart and 1e-3 deep
    (bisection on the restatement); a tetrahedron against a large hull.  Deviations are printed; the assertion is 32 eps x scale."""
    rng = np.random.default_rng(0)
    worst = {"random": 0.0, "touch": 0.0, "tetra": 0.0}
    iters, nsep, nov, nfacet = 0, 0, 0, 0
    for i in range(240):
        tetra = i >= 200
        A = _cloud(rng, 4 if tetra else int(rng.integers(4, 41)), rng.uniform(0.05, 0.3))
        B = _cloud(rng, 40 if tetra else int(rng.integers(4, 41)), 0.5 if tetra else rng.uniform(0.05, 0.3))
        RA, RB = random_rotations(rng, 2)
        cA = rng.standard_normal(3) * 0.3
        cB = cA + rng.standard_normal(3) * (0.15 if i % 2 else 0.5)
        dev, want, it, facet = _deviation(A, B, RA, cA, RB, cB)
        worst["tetra" if tetra else "random"] = max(worst["tetra" if tetra else "random"], dev)
        iters, nsep, nov, nfacet = max(iters, it), nsep + (want > 0), nov + (want <= 0), nfacet + facet
        assert facet == (want <= 0) or abs(want) <= 64 * EPS, (i, want)
        if i % 4 == 0 and not tetra:  # scaled to touch: slide B along the line of centres
            u = (cB - cA) / np.linalg.norm(cB - cA)
            for target in (1e-7, -1e-3):
                lo, hi = -2.0, 3.0  # (the signed distance grows with the shift along u between these: deep inside to far apart)
                f = lambda s: hr.hull_distance(RA, cA, A.vertices, RB, cB + s * u, B.vertices) - target  # noqa: E731
                if not (f(lo) < 0 < f(hi)):
                    continue
                for _ in range(60):
                    mid = 0.5 * (lo + hi)
                    lo, hi = (mid, hi) if f(mid) < 0 else (lo, mid)
                dev, want, it, facet = _deviation(A, B, RA, cA, RB, cB + hi * u)
                assert abs(want - target) <= 1e-9
                worst["touch"] = max(worst["touch"], dev)
                iters = max(iters, it)
                nsep, nov = nsep + (want > 0), nov + (want <= 0)
    print(f"emulation against restatement, eps x scale: {worst}; most GJK iterations {iters}; {nsep} separated, {nov} overlapping")
    assert nsep >= 60 and nov >= 60 and worst["touch"] > 0
    assert max(worst.values()) <= 32.0
    assert 2 * iters <= MAX_ITER  # no evaluation comes near the cap


def test_boxes_as_hulls_equal_the_box_restatement():
    """the random and the exactly parallel box pairs of tests/test_boxes.py through hull_from_box: both branches, the counts asserted"""
    from flobaroid_amd.collision import Box, hull_from_box

    case = all_cases()
    want = br.box_distance(*case)
    worst, iters, nfacet = 0.0, 0, 0
    for i in range(len(want)):
        A, B = hull_from_box(Box("a", case[2][i], np.zeros(3))), hull_from_box(Box("b", case[5][i], np.zeros(3)))
        assert (len(A.vertices), len(A.planes), len(A.edges)) == (8, 6, 12)
        got, it, facet = emul_distance(A, B, case[0][i:i + 1], case[1][i:i + 1], case[3][i:i + 1], case[4][i:i + 1])
        scale = br.pair_scale(case[1][i], case[2][i], case[4][i], case[5][i])  # (|cB - cA| + |hA| + |hB|: below the hulls' own scale)
        worst, iters, nfacet = max(worst, abs(got[0] - want[i]) / (EPS * scale)), max(iters, int(it[0])), nfacet + bool(facet[0])
    print(f"boxes as hulls against the box restatement: {worst:.2f} eps x scale, most iterations {iters}, facet pass {nfacet} of {len(want)}")
    assert (want > 0).sum() >= 100 and (want <= 0).sum() >= 100 and nfacet >= 100 and len(want) - nfacet >= 100
    assert worst <= 32.0 and 2 * iters <= MAX_ITER


def test_nan_pose_is_a_nan():
    rng = np.random.default_rng(1)
    A, B = _cloud(rng, 10, 0.1), _cloud(rng, 12, 0.1)
    R = random_rotations(rng, 2)
    c = np.array([[0.0, 0.0, 0.0], [0.5, np.nan, 0.0]])
    got, _, _ = emul_distance(A, B, R[:1], c[:1], R[1:], c[1:])
    assert np.isnan(got[0]) and np.isnan(hr.hull_distance(R[0], c[0], A.vertices, R[1], c[1], B.vertices))


# ---- the vertex cap, round shapes, an apex of 127 faces, exact contacts (tests/hull_shapes.py) ---------------------------------------------------
GAPS = (1e-2, 1e-6, -1e-6, 1e-9, -1e-9, 1e-12, -1e-12, 0.0, -1e-3)


def _rz(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def _family(name, cases):
    """runs (A, B, RA, cA, RB, cB, tag) through the emulation and the restatement: the file's rule 32 eps x scale, the facet pass exactly
    when the restatement is <= 0 (or within 64 eps of it), a third of the cases on each side of 0 at least, no more than half the cap of
    iterations; returns (worst deviation in eps x scale, most iterations, [restatement's value])"""
    worst, iters, wants, who = 0.0, 0, [], None
    for A, B, RA, cA, RB, cB, tag in cases:
        dev, want, it, facet = _deviation(A, B, np.asarray(RA, dtype=np.float64), np.asarray(cA, dtype=np.float64), np.asarray(RB, dtype=np.float64),
                                          np.asarray(cB, dtype=np.float64))
        if dev > worst:
            worst, who = dev, tag
        iters = max(iters, it)
        wants.append(want)
        assert facet == (want <= 0) or abs(want) <= 64 * EPS, (name, tag, want, facet)
        assert dev <= 32.0, (name, tag, dev, want)
    wants = np.array(wants)
    print(f"{name}: worst |emulation - restatement| = {worst:.3g} eps x scale ({who}); most GJK iterations {iters}; {(wants > 0).sum()} separated, "
          f"{(wants <= 0).sum()} touching or overlapping of {len(wants)}")
    assert 3 * (wants > 0).sum() >= len(wants) and 3 * (wants <= 0).sum() >= len(wants), name
    assert 2 * iters <= MAX_ITER, name
    return worst, iters, wants


def _dyadic_shapes():
    """shapes with dyadic sizes: their tops, bottoms, apexes and ridges have exact z"""
    from flobaroid_amd.collision import Hull

    z = np.zeros(3)
    return {"prism128": Hull("a", hs.prism(64, 0.25, 0.5), z), "hexprism": Hull("a", hs.prism(6, 0.25, 0.5), z), "box": Hull("a", hs.box([0.25, 0.125, 0.5]), z),
            "slab": Hull("a", hs.box([5.0, 5.0, 0.5]), z), "cone128": Hull("a", hs.cone(127, 0.25, 0.5), z), "cube": Hull("a", hs.box([0.25, 0.25, 0.25]), z),
            "bar": Hull("a", hs.box([0.25, 0.125, 0.125]), z), "ridge_y": Hull("a", hs.wedge(0.25, 0.5, 0.25, "y"), z),
            "ridge_x": Hull("a", hs.wedge(0.25, 0.5, 0.25, "x"), z)}


def _stacked(A, B, RB, xy, gap):
    """B in the axes RB above A (identity, at the origin): its lowest point ``gap`` above A's highest, shifted by xy"""
    low = float((B.vertices @ np.asarray(RB).T)[:, 2].min())
    return A, B, np.eye(3), np.zeros(3), RB, np.array([xy[0], xy[1], (float(A.vertices[:, 2].max()) - low) + gap])


def contact_kinds():
    """{kind: (A, B, rotation of B, shift in x and y)}: B's lowest feature straight above A's highest.  z is exact for all but the box on
    its edge (a rotation by pi / 4): there the restatement says where the two are."""
    s = _dyadic_shapes()
    down, side, quarter = hs.TURNS["apex_down"], hs.TURNS["on_side"], hs.TURNS["quarter"]
    return {"edge-edge": (s["ridge_y"], s["ridge_x"], down, (0.0625, -0.03125)), "edge-edge, turned": (s["ridge_y"], s["ridge_x"], _rz(0.3) @ down, (0.0625, -0.03125)),
            "apex-face": (s["cube"], s["cone128"], down, (0.0625, -0.03125)), "apex-apex": (s["cone128"], s["cone128"], down, (0.0, 0.0)),
            "edge-face": (s["cube"], s["bar"], quarter, (0.03125, 0.0625)), "prism side edge on a prism cap": (s["prism128"], s["prism128"], side, (0.03125, 0.0625))}


def test_zoo_tables_at_the_vertex_cap():
    from flobaroid_amd.collision import FBR_MAX_HULL_VERTICES, Hull

    rng = np.random.default_rng(21)
    for kind in hs.KINDS:
        for link in ("l", None):
            h = hs.zoo(rng, link, kind)
            _check_tables(h)  # (Euler's V - E + F = 2 among its checks)
            assert (len(h.vertices), len(h.planes), len(h.edges)) == hs.COUNTS[kind], kind
            assert (h.rot is None) == (link is not None)
    assert max(c[0] for c in hs.COUNTS.values()) == FBR_MAX_HULL_VERTICES == 128
    w = Hull("w", hs.wedge(0.25, 0.5, 0.25, "x"), np.zeros(3))
    _check_tables(w)
    assert (len(w.vertices), len(w.planes), len(w.edges)) == (6, 5, 9)
    for name, h in _dyadic_shapes().items():
        _check_tables(h)
        assert len(h.vertices) - len(h.edges) + len(h.planes) == 2, name
    # the apex of the cone: 127 side faces and 127 edges meet in the last vertex
    c = _dyadic_shapes()["cone128"]
    apex = int(np.argmax(c.vertices[:, 2]))
    assert (c.edges[:, :2] == apex).any(axis=1).sum() == 127


def test_zoo_pairs_in_random_poses():
    """all 64 ordered pairs of the eight kinds (4 to 128 vertices, 1 mm to 10 m), 12 seeded poses each: B's centre along a random direction u
    at 0.55 .. 1.2 x the sum of the two support widths along u (1: the supporting planes touch)"""
    rng = np.random.default_rng(22)
    zoo = {k: hs.zoo(rng, "l", k) for k in hs.KINDS}

    def cases():
        for ka, A in zoo.items():
            for kb, B in zoo.items():
                for i in range(12):
                    RA, RB = random_rotations(rng, 2)
                    u = rng.standard_normal(3)
                    u /= np.linalg.norm(u)
                    reach = float((A.vertices @ RA.T @ u).max() - (B.vertices @ RB.T @ u).min())
                    cA = rng.standard_normal(3) * 0.3 * A.diameter  # (the restatement rounds world coordinates: they stay within the pair's scale)
                    yield A, B, RA, cA, RB, cA + u * reach * rng.uniform(0.55, 1.2), f"{ka} / {kb} pose {i}"

    worst, iters, _ = _family("zoo pairs", cases())
    assert iters > 7  # (beyond what the random clouds above reach)


def test_parallel_stacking():
    """flat bottoms on flat tops, the faces exactly parallel: B as it is and turned about z by 0.3 and pi / 4, at five gaps"""
    s = _dyadic_shapes()

    def cases():
        for ka in ("prism128", "hexprism", "box", "slab"):
            for kb in ("prism128", "hexprism", "box", "slab", "cone128"):
                for a in (0.0, 0.3, np.pi / 4):
                    for xy in ((0.0, 0.0), (0.03125, -0.0625)):
                        for gap in (1e-3, 1e-9, 0.0, -1e-9, -1e-3):
                            yield (*_stacked(s[ka], s[kb], _rz(a), xy, gap), f"{kb} on {ka}, turned {a:.2f}, shift {xy}, gap {gap:g}")

    _, _, wants = _family("parallel stacking", cases())
    gaps = np.tile([1e-3, 1e-9, 0.0, -1e-9, -1e-3], len(wants) // 5)
    assert np.all(np.abs(wants - gaps) <= 1e-13)  # (the minimum translation of a shallow stack is the vertical one)


def test_exact_contacts_by_kind():
    """edge on edge, apex on face, apex on apex, edge on face, a prism's side edge on a prism's cap: from 1e-2 apart to 1e-3 deep"""
    def cases():
        for kind, (A, B, RB, xy) in contact_kinds().items():
            for gap in GAPS:
                yield (*_stacked(A, B, RB, xy, gap), f"{kind}, gap {gap:g}")

    _, _, wants = _family("contact kinds", cases())
    gaps = np.tile(GAPS, len(wants) // len(GAPS))
    # apart: the gap itself; deep: no deeper than the vertical translation that separates the two
    assert np.all(np.abs(wants - gaps)[gaps > 0] <= 1e-14) and np.all(wants[gaps <= 0] <= 64 * EPS) and np.all(wants[gaps <= 0] >= gaps[gaps <= 0] - 1e-14)


# ---- flobaroid_amd/collision.py ----------------------------------------------------------------------------------------------------------
def _write_stl(path, tri, ascii_):
    if ascii_:
        with open(path, "w") as fh:
            fh.write("solid t\n")
            for t in tri:
                fh.write(" facet normal 0 0 0\n  outer loop\n" + "".join(f"   vertex {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}\n" for v in t) + "  endloop\n endfacet\n")
            fh.write("endsolid t\n")
    else:
        with open(path, "wb") as fh:
            fh.write(b"\0" * 80 + struct.pack("<I", len(tri)))
            for t in tri:
                fh.write(struct.pack("<12fH", 0, 0, 0, *t.reshape(-1), 0))


CUBE_TRI = np.array([[[0, 0, 0], [1, 1, 0], [1, 0, 0]], [[0, 0, 0], [0, 1, 0], [1, 1, 0]], [[0, 0, 1], [1, 0, 1], [1, 1, 1]], [[0, 0, 1], [1, 1, 1], [0, 1, 1]],
                     [[0, 0, 0], [1, 0, 0], [1, 0, 1]], [[0, 0, 0], [1, 0, 1], [0, 0, 1]], [[0, 1, 0], [1, 1, 1], [1, 1, 0]], [[0, 1, 0], [0, 1, 1], [1, 1, 1]],
                     [[0, 0, 0], [0, 1, 1], [0, 1, 0]], [[0, 0, 0], [0, 0, 1], [0, 1, 1]], [[1, 0, 0], [1, 1, 0], [1, 1, 1]], [[1, 0, 0], [1, 1, 1], [1, 0, 1]]],
                    dtype=np.float64) * np.array([0.25, 0.5, 0.125])


def test_read_stl_binary_and_ascii(tmp_path):
    from flobaroid_amd.collision import Hull, read_stl

    _write_stl(tmp_path / "b.stl", CUBE_TRI, False)
    _write_stl(tmp_path / "a.stl", CUBE_TRI, True)
    b, a = read_stl(tmp_path / "b.stl"), read_stl(tmp_path / "a.stl")
    assert b.shape == (12, 3, 3) and b.dtype == np.float64 and np.array_equal(a, b) and np.array_equal(b, CUBE_TRI)
    (tmp_path / "m.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with pytest.raises(ValueError, match="m.obj"):
        read_stl(tmp_path / "m.obj")
    for name, count in MESHES.items():
        tri = read_stl(os.path.join(URDF, "meshes", "walkman", "simple", name + ".STL"))
        assert tri.ndim == 3 and tri.shape[1:] == (3, 3) and np.isfinite(tri).all()
        assert len(Hull(name, tri.reshape(-1, 3) * 0.001, np.zeros(3)).vertices) == count, name


def _check_tables(h):
    V, F, E = h.vertices, h.planes, h.edges
    d = h.diameter
    assert np.abs(np.linalg.norm(F[:, :3], axis=1) - 1.0).max() <= 1e-12
    assert (V @ F[:, :3].T - F[:, 3]).max() <= 1e-9 * d                      # every vertex inside every plane
    assert (E[:, 2] != E[:, 3]).all() and (E[:, 0] != E[:, 1]).all()
    for k in (0, 1):                                                         # both ends of an edge on both of its faces
        for f in (2, 3):
            assert np.abs(np.einsum("ij,ij->i", V[E[:, k]], F[E[:, f], :3]) - F[E[:, f], 3]).max() <= 1e-9 * d
    assert len(V) - len(E) + len(F) == 2                                     # Euler, on merged faces
    assert len({tuple(sorted(e[:2])) for e in E.tolist()}) == len(E)


def test_hull_tables():
    from flobaroid_amd.collision import Box, Hull, hull_from_box

    rng = np.random.default_rng(3)
    for n in (4, 5, 17, 40):
        _check_tables(_cloud(rng, n, 0.2))
    cube = Hull("cube", CUBE_TRI.reshape(-1, 3), np.zeros(3))  # 12 triangles, coplanar in pairs
    _check_tables(cube)
    assert (len(cube.vertices), len(cube.planes), len(cube.edges)) == (8, 6, 12)
    # points inside a face and on an edge are no vertices
    extra = np.concatenate([CUBE_TRI.reshape(-1, 3), [[0.125, 0.25, 0.0], [0.125, 0.0, 0.0], [0.1, 0.2, 0.05]]])
    h = Hull("cube+", extra, np.zeros(3))
    _check_tables(h)
    assert len(h.planes) == 6
    b = hull_from_box(Box(None, np.array([0.1, 0.2, 0.3]), np.array([1.0, 2.0, 3.0]), np.eye(3), "w"))
    _check_tables(b)
    assert b.link_name is None and b.name == "w" and np.array_equal(b.offset, [1, 2, 3]) and np.array_equal(np.abs(b.vertices).max(0), [0.1, 0.2, 0.3])
    for bad in (np.zeros((3, 3)), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0.0]], dtype=float)):
        with pytest.raises(ValueError):
            Hull("flat", bad, np.zeros(3))
    for name in MESHES:
        from flobaroid_amd.collision import read_stl

        _check_tables(Hull(name, read_stl(os.path.join(URDF, "meshes", "walkman", "simple", name + ".STL")).reshape(-1, 3) * 0.001, np.zeros(3)))


def left_arm_hulls(**kw):
    from flobaroid_amd.collision import hulls_from_urdf

    topo = load_topo("walkman_left_arm")
    return topo, hulls_from_urdf(os.path.join(URDF, "walkman_left_arm.urdf"), topo.link_names, **kw)


def test_hulls_from_urdf_on_the_left_arm(tmp_path):
    import shutil
    import xml.etree.ElementTree as ET

    from flobaroid_amd.collision import Box, hulls_from_urdf, read_stl, world_hulls_from_urdf, world_boxes_from_urdf

    topo, (hulls, box_links) = left_arm_hulls()
    urdf = os.path.join(URDF, "walkman_left_arm.urdf")
    tree = ET.parse(urdf)
    assert box_links == [] and len(hulls) == 9 and list(hulls) == [n for n in topo.link_names if n in hulls]
    for link in tree.findall("link"):
        name = link.attrib["name"]
        mesh = link.find("collision/geometry/mesh")
        if mesh is None:
            assert name not in hulls
            continue
        h = hulls[name]
        stem = os.path.basename(mesh.attrib["filename"])[:-4]
        scale = np.array([float(v) for v in mesh.attrib["scale"].split()])
        pts = read_stl(os.path.join(URDF, "meshes", "walkman", "simple", stem + ".STL")).reshape(-1, 3)
        assert len(h.vertices) == MESHES[stem] and h.link_name == name and h.rot is None
        # the vertices are mesh vertices times the scale, signs included: a negative y scale mirrors them
        assert all(np.abs(pts * scale - v).sum(1).min() == 0.0 for v in h.vertices)
        if scale[1] < 0:
            assert np.array_equal(h.bounds[:, 1], [(pts[:, 1] * scale[1]).min(), (pts[:, 1] * scale[1]).max()]) and h.bounds[0, 1] == -pts[:, 1].max() * 0.001
        assert np.array_equal(h.bounds, [(pts * scale).min(0), (pts * scale).max(0)])
        vo = link.find("visual/origin")
        assert np.array_equal(h.offset, [float(v) for v in vo.attrib.get("xyz", "0 0 0").split()] if vo is not None else np.zeros(3))
    assert sum(float(m.attrib["scale"].split()[1]) < 0 for m in tree.findall("link/collision/geometry/mesh")) >= 1
    # the cap names the link and the count
    with pytest.raises(ValueError, match=r"LShy.*52"):
        left_arm_hulls(max_vertices=50)
    # a missing file (here: all but one) sends the link to box_links, with the cube around the a-priori centre of mass when asked for; the
    # visual origin, rotated or not, gives the offset
    shutil.copytree(URDF, tmp_path / "urdf", ignore=shutil.ignore_patterns("*.STL"))
    os.makedirs(tmp_path / "urdf" / "meshes" / "walkman" / "simple", exist_ok=True)
    shutil.copy(os.path.join(URDF, "meshes", "walkman", "simple", "Elbow.STL"), tmp_path / "urdf" / "meshes" / "walkman" / "simple")
    text = open(urdf).read()
    moved = str(tmp_path / "urdf" / "walkman_left_arm.urdf")
    root = ET.fromstring(text)
    for link in root.findall("link"):
        if link.attrib["name"] == "LElb":
            ET.SubElement(link.find("visual"), "origin", {"xyz": "0.01 -0.02 0.03", "rpy": "0.1 0.2 0.3"}) if link.find("visual/origin") is None else \
                link.find("visual/origin").attrib.update({"xyz": "0.01 -0.02 0.03", "rpy": "0.1 0.2 0.3"})
    ET.ElementTree(root).write(moved)
    x = topo.x_std()
    got, bl = hulls_from_urdf(moved, topo.link_names, x_std=x, cube_size=0.1, scale=0.5)
    assert set(bl) == set(hulls) - {"LElb"} and set(got) == set(hulls)
    assert np.array_equal(got["LElb"].offset, [0.01, -0.02, 0.03]) and np.array_equal(got["LElb"].vertices, hulls["LElb"].vertices)  # (not rotated)
    i = list(topo.link_names).index("LShy")
    assert len(got["LShy"].vertices) == 8 and np.allclose(np.abs(got["LShy"].vertices), 0.025) and np.allclose(got["LShy"].offset, 0.5 * x[10 * i + 1:10 * i + 4] / x[10 * i])
    assert hulls_from_urdf(moved, topo.link_names)[0].keys() == {"LElb"}
    # world links are boxes in both placements
    w = os.path.join(URDF, "world_walkman_suspended.urdf")
    for placement in ("reference", "geometric"):
        wh, wb = world_hulls_from_urdf(w, placement), world_boxes_from_urdf(w, placement)
        assert list(wh) == list(wb)
        for n in wh:
            assert wh[n].link_name is None and wh[n].name == n and np.array_equal(wh[n].offset, wb[n].center) and np.array_equal(wh[n].rot, wb[n].rot)
            assert np.array_equal(np.abs(wh[n].vertices).max(0), wb[n].half) and len(wh[n].edges) == 12


@pytest.mark.parametrize("cfg", [{"worldCollisionMargin": 0.03}, {"ignoreLinksForCollision": ["LShr"], "ignoreLinkPairsForCollision": [["crane_tip", "LElb"]]}])
def test_collision_set_with_hulls(cfg):
    from flobaroid_amd.collision import collision_pairs, collision_set, world_hulls_from_urdf

    topo, (hulls, _) = left_arm_hulls()
    wh = world_hulls_from_urdf(os.path.join(URDF, "world_walkman_suspended.urdf"))
    cs = collision_set(topo, {}, dict(cfg, collisionMode="convex"), hulls=hulls, world_hulls=wh)
    want = collision_pairs(topo, {}, cfg, world_links=list(wh), boxes=hulls)
    assert cs["pair_names"] == want and len(want) > 16 and cs["offset_in_link_axes"] is False
    assert cs["pair_names"] == collision_set(topo, {}, cfg, hulls=hulls, world_hulls=wh)["pair_names"]  # (convex is the default with hulls)
    assert np.all(cs["columns"][:, 0] == 2) and sorted(cs["columns"][:, 1]) == list(range(len(want)))
    assert [h.link_name or h.name for h in cs["hulls"]] == [n for n in topo.link_names if n in hulls] + list(wh)
    for (a, b), col in zip(want, cs["columns"][:, 1]):
        ha, hb = (cs["hulls"][i] for i in cs["hull_pairs"][col])
        assert (ha.link_name or ha.name, hb.link_name or hb.name) == (a, b)
    assert np.all(np.diff(cs["hull_pairs"][:, 0]) >= 0)  # a pair's first hull changes rarely
    assert np.array_equal(cs["margins"], [cfg.get("worldCollisionMargin", 0.0) if (a in wh or b in wh) else 0.0 for a, b in want])
    assert np.array_equal(collision_set(topo, {}, cfg, margins=np.arange(len(want)), hulls=hulls, world_hulls=wh)["margins"], np.arange(len(want)))
    # without hulls= the mode is refused as before; the triangle-mesh modes are refused by name
    with pytest.raises(ValueError, match="'capsule' and 'box'"):
        collision_set(topo, {}, {"collisionMode": "convex"}, boxes={}, world_boxes={})
    with pytest.raises(ValueError, match="LElb"):
        collision_set(topo, {}, dict(cfg, fullMeshLinks=["LElb"]), hulls=hulls, world_hulls=wh)
    with pytest.raises(ValueError, match="full"):
        collision_set(topo, {}, dict(cfg, collisionMode="full"), hulls=hulls, world_hulls=wh)
    with pytest.raises(ValueError):
        collision_set(topo, {}, dict(cfg, collisionMode="box"), hulls=hulls, world_hulls=wh)


# ---- excitation: the collision block in convex mode ------------------------------------------------------------------------------------------
class HostHullEngine:
    """candidate_hull_distances from the restatement: what excitation._collision_block needs of an Engine in convex mode"""

    def __init__(self, topo, floating):
        self.topo, self.floating, self.n, self.calls = topo, floating, topo.num_dofs, []

    def set_capsules(self, *a, **k):
        raise AssertionError("convex mode installs no capsules")

    set_boxes = set_capsules

    def set_hulls(self, hulls, pairs, offset_in_link_axes=False):
        self.hulls, self.pairs, self.mode = as_tuples(self.topo, hulls), np.asarray(pairs).reshape(-1, 2), offset_in_link_axes
        self.calls.append("set_hulls")

    def candidate_hull_distances(self, st, ncand, step=3, base_pos=None, device_out=None):
        S = st["q"].shape[0]
        T = S // ncand
        rows = [c * T + i for c in range(ncand) for i in range(0, T, step)]
        R, c = hr.hull_world(self.topo, self.hulls, st["q"], self.floating, st.get("rpy"), base_pos, self.mode)
        val, idx = hr.candidate_minimum(hr.pair_distances(R, c, self.hulls, self.pairs, rows)[0], ncand, step)
        self.calls.append(("hull_distances", S, step))
        return {"dist": val, "idx": idx}


def small_hull_set(rng, margin=0.02):
    """threeLinks with a box hull on every link and the floor of world_kuka.urdf lifted among them: [topo, collision set]"""
    from flobaroid_amd.collision import Box, collision_set, hull_from_box, world_hulls_from_urdf
    from test_boxes import synthetic_boxes

    topo = load_topo("threeLinks")
    hulls = {topo.link_names[l]: hull_from_box(Box(topo.link_names[l], h, c)) for l, h, c, _ in synthetic_boxes(topo, rng)}
    wh = world_hulls_from_urdf(os.path.join(URDF, "world_kuka.urdf"), "geometric")
    wh["ground_link"].offset = wh["ground_link"].offset + np.array([0.0, 0.0, 0.3])
    return topo, collision_set(topo, {}, {"collisionMode": "convex", "worldCollisionMargin": margin}, hulls=hulls, world_hulls=wh)


def restate_hull_block(topo, floating, cs, q, config, rpy=None, bpos=None):
    """the reference's collision loop for ONE candidate, sample by sample, on the hull restatement: (g (P,), {pair: the winning sample, or
    minus the count of the winning transition configuration}, {pair: the reference's argmin, which only a trajectory sample updates})"""
    hulls, P = as_tuples(topo, cs["hulls"]), len(cs["pair_names"])
    pairs = cs["hull_pairs"][cs["columns"][:, 1]]  # in the order of pair_names
    mode = bool(cs.get("offset_in_link_axes", False))
    g, argmin, main = np.full(P, 1e10), {}, {}

    def dists(qrow, r, b):
        R, c = hr.hull_world(topo, hulls, qrow[None], floating, None if r is None else r[None], None if b is None else b[None], mode)
        return hr.pair_distances(R, c, hulls, pairs)[0][0] - cs["margins"]

    T = q.shape[0]
    for i in range(0, T, int(config.get("collisionCheckStep", 3))):
        d = dists(q[i], None if rpy is None else rpy[i], None if bpos is None else bpos[i])
        for k in range(P):
            if d[k] < g[k]:
                g[k], argmin[k], main[k] = d[k], i, i
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
                    d = dists(s * qb, None if rpy is None else rpy[pz], None if bpos is None else bpos[pz])
                    for k in range(P):
                        if d[k] < g[k]:
                            g[k], argmin[k] = d[k], -count
    return g, argmin, main


def test_convex_collision_block_with_a_host_engine():
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(5)
    topo, cs = small_hull_set(rng)
    C, T, n = 2, 16, topo.num_dofs
    st = random_states(topo, C * T, rng, False, use_limits=True)
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 3, "collisionMode": "convex"}
    eng = HostHullEngine(topo, False)
    coll = exc._collision_block(eng, st, C, config, cs)
    assert eng.calls == ["set_hulls", ("hull_distances", C * T, 3), ("hull_distances", C * 2 * 3, 1)]  # the main trajectory, then the transitions
    P = len(cs["pair_names"])
    assert coll["g"].shape == (C, P)
    for c in range(C):
        g, argmin, main = restate_hull_block(topo, False, cs, st["q"][c * T:(c + 1) * T], config)
        assert np.abs(coll["g"][c] - g).max() <= 1e-13
        assert all(coll["idx"][c, k] == argmin.get(k, -1) and coll["argmin"][c, k] == main.get(k, -1) for k in range(P))
    # the keyword of the public function selects the hull call; boxes= keeps working and the two exclude each other
    part = exc.candidate_collision_constraints(eng, st, C, config, hulls=True)
    assert np.array_equal(part["dist"], coll["dist"][:, np.argsort(cs["columns"][:, 1])])
    with pytest.raises(ValueError):
        exc.candidate_collision_constraints(eng, st, C, config, hulls=True, boxes=True)
    # convex mode without hulls, hulls in another mode, and the gradient entry points
    with pytest.raises(ValueError, match="collisionMode 'convex' needs a collision set with hulls"):
        exc._collision_block(eng, st, C, config, {"capsules": [], "pairs": np.zeros((0, 2))})
    with pytest.raises(ValueError, match="hull pairs"):
        exc._collision_block(eng, st, C, dict(config, collisionMode="box"), cs)
    with pytest.raises(ValueError):
        exc._collision_block(eng, st, C, dict(config, collisionMode="full"), cs)
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    for kw in ({}, {"box_gradient": True}):
        with pytest.raises(ValueError, match="no mesh code"):
            exc.candidate_collision_gradient(eng, st, C, [], 50.0, config, cs, **kw)
        for mode in ("capsule", "box") if kw else ("capsule",):
            with pytest.raises(ValueError, match="hull pairs"):
                exc.candidate_collision_gradient(eng, st, C, [], 50.0, dict(config, collisionMode=mode), cs, **kw)
        with pytest.raises(ValueError, match="hull pairs"):
            exc.candidate_gradients_from_coefficients(eng, [], T, 50.0, None, None, limits, topo.dof_names, config, collision=cs, **kw)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_hull_symbols_in_header_binding_and_library():
    from flobaroid_amd import _lib

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    for name in ("fbr_model_set_hulls", "fbr_candidate_hull_distances"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr), name
    assert lib.fbr_version() == _lib.FBR_VERSION == 104
    limits = {k: int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) for k in ("FBR_MAX_HULLS", "FBR_MAX_HULL_PAIRS", "FBR_MAX_HULL_VERTICES")}
    assert limits == {"FBR_MAX_HULLS": 4096, "FBR_MAX_HULL_PAIRS": 262144, "FBR_MAX_HULL_VERTICES": 128}
    from flobaroid_amd import collision

    assert collision.FBR_MAX_HULL_VERTICES == limits["FBR_MAX_HULL_VERTICES"] >= max(MESHES.values())
    assert all(hasattr(_lib.Engine, a) for a in ("set_hulls", "candidate_hull_distances"))
    assert lib.fbr_model_set_hulls(None, 0, None, None, None, 0, None, None, None, None, None, None, 0, None) == -1  # FBR_E_INVALID: no model


def _validate(L, hulls, link, pairs, edit=None, rot=True):
    """the checks of fbr_model_set_hulls (the same text, tests/emul/hull_emul.cpp): (0 or -1, message)"""
    vbeg, v, fbeg, pl, ebeg, ed, _ = tables(hulls)
    arr = {"link": _c(link, np.int32), "offset": _c([h.offset for h in hulls]).reshape(-1), "rot": _c([np.eye(3)] * len(hulls)).reshape(-1),
           "vbeg": vbeg, "verts": v.copy(), "fbeg": fbeg, "planes": pl.copy(), "ebeg": ebeg, "edges": ed.copy(), "pairs": _c(pairs, np.int32).reshape(-1, 2)}
    if edit:
        edit(arr)
    msg = ctypes.create_string_buffer(256)
    rc = emul().hull_validate(L, len(arr["link"]), _p(arr["link"]), _p(arr["offset"]), _p(arr["rot"]) if rot else None, _p(arr["vbeg"]), _p(arr["verts"]),
                              _p(arr["fbeg"]), _p(arr["planes"]), _p(arr["ebeg"]), _p(arr["edges"]), len(arr["pairs"]), _p(arr["pairs"]), msg, 256)
    return rc, msg.value.decode()


def test_set_hulls_refuses_what_the_header_lists():
    """fbr_hull_validate is what fbr_model_set_hulls runs before it touches the set in place (tests/test_gpu_hulls.py: the set survives)"""
    rng = np.random.default_rng(2)
    hulls = [_cloud(rng, 12, 0.1), _cloud(rng, 9, 0.1), _cloud(rng, 6, 0.1), _cloud(rng, 5, 0.1)]
    link, pairs, L = [0, 2, -1, -1], [[0, 1], [0, 2], [1, 3]], 3
    assert _validate(L, hulls, link, pairs) == (0, "")

    def put(key, index, value):
        def edit(arr):
            arr[key].reshape(-1)[index] = value
        return edit

    bad = {
        "link index": dict(edit=put("link", 1, 3)), "link below -1": dict(edit=put("link", 1, -2)),
        "pair index": dict(edit=put("pairs", 1, 4)), "negative pair index": dict(edit=put("pairs", 0, -1)),
        "paired with itself": dict(edit=put("pairs", 1, 0)), "two world hulls": dict(edit=put("pairs", 4, 2)),
        "non-finite vertex": dict(edit=put("verts", 5, np.nan)), "non-finite offset": dict(edit=put("offset", 2, np.inf)),
        "non-finite plane": dict(edit=put("planes", 3, np.nan)), "non-finite rotation": dict(edit=put("rot", 9 * 2 + 4, np.nan)),
        "a world hull needs rot": dict(rot=False),
        "not unit": dict(edit=lambda a: a["planes"].reshape(-1, 4).__setitem__((0, slice(0, 3)), a["planes"].reshape(-1, 4)[0, :3] * (1 + 1e-8))),
        "outside face": dict(edit=lambda a: a["verts"].reshape(-1, 3).__setitem__(0, a["verts"].reshape(-1, 3)[0] * 1.001)),
        "two faces are the same": dict(edit=lambda a: a["edges"].reshape(-1, 4).__setitem__((2, 3), a["edges"].reshape(-1, 4)[2, 2])),
        "edge vertex index": dict(edit=put("edges", 0, 12)), "edge face index": dict(edit=put("edges", 2, 99)),
    }
    for why, kw in bad.items():
        rc, msg = _validate(L, hulls, link, pairs, **kw)
        assert rc == -1 and msg, why
    assert "unit" in _validate(L, hulls, link, pairs, **bad["not unit"])[1] and "outside" in _validate(L, hulls, link, pairs, **bad["outside face"])[1]
    assert "same" in _validate(L, hulls, link, pairs, **bad["two faces are the same"])[1]
    # a vertex 1e-10 x the diameter outside is within the tolerance
    assert _validate(L, hulls, link, pairs, edit=lambda a: a["verts"].reshape(-1, 3).__setitem__(0, a["verts"].reshape(-1, 3)[0] * (1 + 1e-11)))[0] == 0
    # the limits: hulls, pairs, vertices of one hull
    from flobaroid_amd.collision import Hull

    t = np.linspace(0, 2 * np.pi, 65, endpoint=False)
    ring = np.concatenate([np.stack([np.cos(t), np.sin(t), np.full(65, z)], 1) for z in (-0.5, 0.5)])  # a prism of 130 vertices
    big = Hull("big", ring, np.zeros(3))
    assert len(big.vertices) == 130 and "130 vertices" in _validate(L, [big], [0], [])[1]
    assert _validate(L, [hulls[0]] * 4097, [0] * 4097, [])[0] == -1
    assert _validate(L, hulls, link, [[0, 1]] * 262145)[0] == -1
