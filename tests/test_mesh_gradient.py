"""The mesh distance gradient off the GPU: the HIP-free text of csrc/fbr_mesh_grad.h (g++, tests/emul/mesh_grad_emul.cpp) against the NumPy /
Qhull restatement (tests/mesh_gradient_restatement.py: whole re-walks, every joint, Qhull and closed forms).  The emulation of record is the
single pass -- fbr_rigidgrad_item with fbr_mesh_distance as its functor --; the device's route (recorded poses, one distance per stencil
point, the slot table, the quotients of stage C) is held to it bit for bit, with the culling and without.  Then: contacts of known slope on
the gantry; the reason for the feature (a tetrahedron inside the U-channel: the hull gradient pushes, the mesh gradient does not); the
restatement against a Richardson-extrapolated difference; the mesh_gradient=True path of excitation against a host engine; the symbol; the
end-to-end experiment with the restatement alone, which fixes the bar of tests/test_gpu_mesh_gradient.py.

Measured figures are in the docstrings of the tests that print them."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import hull_gradient_restatement as hg
import hull_restatement as hr
import hull_shapes as hs
import mesh_gradient_restatement as mg
import mesh_restatement as mr
import test_hull_gradient as thg
from common import ROOT
from test_box_gradient import ROBOTS, T, item_arrays
from test_hulls import _c, _p, as_tuples, link_index, tables
from test_meshes import box_triangles, mesh_tables, u_channel

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "mesh_grad_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libmesh_grad_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_lib = None
EPS = hg.EPS
KINDS = ("triangle", "soup4", "soup12", "tetra", "channel")


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC, os.path.join(ROOT, "include", "fbr.h")] + [os.path.join(_CSRC, h) for h in (
            "fbr_mesh_grad.h", "fbr_mesh.h", "fbr_hull_grad.h", "fbr_hull.h", "fbr_box_grad.h", "fbr_box.h", "fbr_capsule_grad.h", "fbr_capsule.h",
            "fbr_math.h", "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


def emul_items(topo, floating, hulls, meshes, item_pairs, q, rpy, base_pos, mode, eps, route=0, cull=True):
    """(dist (M,), grad (M, n), stencil points (M,)) of one pair per configuration from the library's own text on the CPU.  ``hulls``:
    flobaroid_amd.collision.Hull objects; ``meshes``: {hull index: triangles}; ``route`` 0: the single pass, 1: the device's stages"""
    parent, dof, jt = _c(topo.parent, np.int32), _c(topo.dof_index, np.int32), _c(topo.joint_type, np.int32)
    rR, rp, ax = _c(topo.rest_R).reshape(-1), _c(topo.rest_p).reshape(-1), _c(topo.axis).reshape(-1)
    link = _c(link_index(topo, hulls), np.int32)
    off = _c([h.offset for h in hulls]).reshape(-1)
    rot = _c([np.eye(3) if h.rot is None else h.rot for h in hulls]).reshape(-1)
    vbeg, v, fbeg, pl, ebeg, ed, _ = tables(hulls)
    mtab, tris = mesh_tables(len(hulls), meshes)
    pr = _c(item_pairs, np.int32).reshape(-1)
    q = _c(q)
    M = q.shape[0]
    rpy = None if rpy is None or not floating else _c(rpy)
    bp = None if base_pos is None or not floating else _c(base_pos)
    dist, grad, ns = np.zeros(M), np.full((M, topo.num_dofs), np.nan), np.zeros(M, dtype=np.int32)
    rc = emul().meshgrad_eval(topo.num_links, topo.num_dofs, _p(parent), _p(dof), _p(rR), _p(rp), _p(ax), _p(jt), int(floating), len(hulls), _p(link),
                              _p(off), _p(rot), int(mode), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), _p(mtab), _p(tris),
                              ctypes.c_long(len(tris)), ctypes.c_double(eps), ctypes.c_long(M), _p(pr), _p(q), _p(rpy), _p(bp), int(route), int(cull),
                              _p(dist), _p(grad), _p(ns))
    assert rc == 0, rc
    return dist, grad, ns


def emul_evaluate(case, C, sample, scale, pose, eps, mode, pairs=None, route=0, cull=True, meshes=None):
    """the contract of fbr_mesh_distance_gradients from the emulation: (dist (C, P), grad (C, P, n))"""
    topo, fl = case["topo"], case["floating"]
    pairs = case["pairs"] if pairs is None else pairs
    meshes = case["meshes"] if meshes is None else meshes
    P, Tn = len(pairs), case["q"].shape[0] // C
    sample = np.asarray(sample).reshape(C, P)
    ps = sample if pose is None else np.where(np.asarray(pose) < 0, sample, pose)
    sc = np.ones((C, P)) if scale is None else np.asarray(scale)
    base = (np.arange(C) * Tn)[:, None]
    rq, rp = (base + np.maximum(sample, 0)).reshape(-1), (base + np.maximum(ps, 0)).reshape(-1)
    dist, grad, _ = emul_items(topo, fl, case["hulls"], meshes, np.tile(pairs, (C, 1)), case["q"][rq] * sc.reshape(-1, 1), case["rpy"][rp] if fl else None,
                               case["bp"][rp] if fl else None, mode, eps, route, cull)
    none = sample < 0
    return np.where(none, mg.NONE, dist.reshape(C, P)), np.where(none[..., None], 0.0, grad.reshape(C, P, -1))


# ---- the cases (shared with tests/test_gpu_mesh_gradient.py) ---------------------------------------------------------------------------------
def mesh_shape(rng, kind, half):
    """triangles (T, 3, 3) of one of KINDS within about the half extents ``half``: a single triangle, soups of 4 and 12 triangles, the
    closed tetrahedron, the three-slab U-channel of tests/test_meshes.py (36 triangles)"""
    half = np.asarray(half, dtype=np.float64)
    if kind == "triangle":
        return rng.standard_normal((1, 3, 3)) * half
    if kind in ("soup4", "soup12"):
        n = int(kind[4:])
        return rng.standard_normal((n, 1, 3)) * half * 0.6 + rng.standard_normal((n, 3, 3)) * half * 0.4
    if kind == "tetra":
        p = rng.standard_normal((4, 3)) * half
        return np.array([[p[a], p[b], p[c]] for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))])
    assert kind == "channel"
    return np.asarray(u_channel().triangles).reshape(-1, 3, 3) * (half / np.array([0.5, 1.0, 0.5]))


def hull_around(link_name, tris, offset, pad, name=None):
    """the Hull of a mesh's points and of the corners of their bounding box grown by ``pad`` (a single triangle has no hull of its own)"""
    from flobaroid_amd.collision import Hull

    pts = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    lo, hi = pts.min(0) - pad, pts.max(0) + pad
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    return Hull(link_name, np.concatenate([pts, corners]), offset, None, name)


def pair_classes(tuples, meshes, pairs):
    """per pair: "mm" two meshes, "mh" / "hm" a mesh and a robot hull (the meshed hull first / second), "mw" / "wm" a mesh and a world hull
    (the world hull second / first), "plain" no mesh"""
    out = []
    for a, b in np.asarray(pairs).reshape(-1, 2):
        ma, mb, wa, wb = int(a) in meshes, int(b) in meshes, tuples[a][0] < 0, tuples[b][0] < 0
        out.append("mm" if ma and mb else "plain" if not (ma or mb) else ("mw" if wb else "mh") if ma else ("wm" if wa else "hm"))
    return out


def make_case(robot, C=3, per_class=2, shift=0):
    """tests/test_hull_gradient.make_case (a small hull on every link, three world hulls, its pairs) with two of every three robot hulls
    replaced by a mesh of KINDS in turn (at most five) inside a hull of its own, and at most ``per_class`` pairs of each of pair_classes"""
    base = thg.make_case(robot, C=C, max_pairs=None)
    topo, hulls = base["topo"], list(base["hulls"])
    rng = np.random.default_rng(100 + base["seed"])
    meshes, count = {}, 0
    for i, h in enumerate(hulls):
        if h.link_name is None or i % 3 == 2 or count == len(KINDS):
            continue
        half = 0.5 * (h.vertices.max(0) - h.vertices.min(0))
        tris = mesh_shape(rng, KINDS[(count + shift) % len(KINDS)], half)
        hulls[i] = hull_around(h.link_name, tris, h.offset, 0.1 * float(half.min()))
        meshes[i] = tris
        count += 1
    tup = as_tuples(topo, hulls)
    cls = np.array(pair_classes(tup, meshes, base["pairs"]))
    keep = np.sort(np.concatenate([np.nonzero(cls == k)[0][:per_class] for k in ("mm", "mh", "hm", "mw", "wm", "plain")]))
    return dict(base, hulls=hulls, tuples=tup, meshes=meshes, pairs=np.ascontiguousarray(base["pairs"][keep]), classes=[str(x) for x in cls[keep]],
                kinds=[KINDS[(j + shift) % len(KINDS)] for j in range(count)])


SHIFT = {"threeLinks": 3, "kuka_lwr4": 0, "walkman_left_arm": 2, "random": 4}  # (so that the two meshes of threeLinks are the closed shapes)


@functools.lru_cache(maxsize=None)
def case_of(robot):
    return make_case(robot, shift=SHIFT[robot])


def reference(case, C, pairs, sample, scale, pose, eps, mode, meshes=None):
    """the restatement with the bars for the emulation's deviation on the same items: (ref, emulated dist, emulated grad).  Asserted: every
    stencil point of a mesh pair is a clear gap or a clear intersection."""
    meshes = case["meshes"] if meshes is None else meshes
    ref = mg.evaluate(case["topo"], case["tuples"], meshes, pairs, case["floating"], case["q"], case["rpy"], case["bp"], C, sample, scale, pose, eps, mode)
    ed, eg = emul_evaluate(case, C, sample, scale, pose, eps, mode, pairs, meshes=meshes)
    fin = np.isfinite(ref["dist"])
    assert np.array_equal(fin, np.isfinite(ed))
    dev = float(np.abs(ed - ref["dist"])[fin & ~ref["none"]].max())
    ref = mg.with_dev(ref, dev)
    assert mg.clear_verdicts(ref).all(), "a stencil point of a mesh pair within 100 bars of contact: change the case"
    return ref, ed, eg


@functools.lru_cache(maxsize=None)
def robot_reference(robot, mode, eps):
    """(case, sample, scale, pose, ref, emulated dist, emulated grad) of the robot's case: the scaled items at eps = 1e-4, the plain ones at 1e-7"""
    case = case_of(robot)
    C, P = case["C"], len(case["pairs"])
    sample, scale, pose = item_arrays(case, np.random.default_rng(11), C, P, eps == 1e-4)
    return (case, sample, scale, pose) + reference(case, C, case["pairs"], sample, scale, pose, eps, mode)


@pytest.mark.parametrize("eps", [1e-7, 1e-4])
@pytest.mark.parametrize("mode", [False, True], ids=["world-axes", "link-axes"])
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_library_text_equals_the_restatement(robot, mode, eps):
    """The single pass within ``bar`` of the restatement entry by entry, the centre distance within its bar, entries the stencil never
    touches exactly 0.0; gaps and contacts both occur among the mesh pairs of the four robots (asserted in the test below).
    Measured (g++ 13, x86-64), largest |emulation - restatement| / bar over both modes and steps: threeLinks 0.011, kuka_lwr4 0.026,
    walkman_left_arm 0.019, random tree 0.013."""
    case, sample, scale, pose, ref, ed, eg = robot_reference(robot, mode, eps)
    live = ~ref["none"]
    worst = (np.abs(eg - ref["grad"]) / ref["bar"]).max()
    print(f"{robot} mode {int(mode)} eps {eps:g}: classes {case['classes']}, meshes {case['kinds']}, contacts "
          f"{int((ref['dist'][live][np.tile(ref['meshed'], (case['C'], 1))[live]] == 0).sum())}, max |delta grad| / bar = {worst:.3f}, "
          f"max |grad| = {np.abs(ref['grad']).max():.3f}")
    assert np.all(np.abs(ed - ref["dist"])[live] <= ref["dist_bar"][live]) and np.all(ed[~live] == mg.NONE)
    assert np.all(np.abs(eg - ref["grad"]) <= ref["bar"])
    assert np.all(eg[~ref["on_path"]] == 0.0) and np.all(eg[~live] == 0.0)
    assert np.all(ed[live][np.tile(ref["meshed"], (case["C"], 1))[live]] >= 0.0), "a mesh distance is never negative"
    assert ref["on_path"].any() and np.abs(ref["grad"]).max() > 1e-2
    if not mode:  # a joint above both links is evaluated in world-axes mode: the two links of some pair share a moving ancestor
        tup = case["tuples"]
        both = [hg.path_dofs(case["topo"], tup[a][0], tup[b][0], False) & ~hg.path_dofs(case["topo"], tup[a][0], tup[b][0], True) for a, b in case["pairs"]]
        assert robot in ("threeLinks", "random") or np.any(both)  # (the two serial arms have such pairs)


def test_the_cases_cover_the_pair_kinds_and_the_meshes():
    kinds, classes = set(), set()
    for robot in ROBOTS:
        case = case_of(robot)
        kinds |= set(case["kinds"])
        classes |= set(case["classes"])
        assert "plain" in case["classes"] and len(case["pairs"]) <= 12 and max(len(t) for t in case["meshes"].values()) <= 36
    assert kinds == set(KINDS) and classes == {"mm", "mh", "hm", "mw", "wm", "plain"}
    contact = gap = 0
    for robot in ROBOTS:
        ref = robot_reference(robot, False, 1e-7)[4]
        m = np.tile(ref["meshed"], (ref["dist"].shape[0], 1)) & ~ref["none"]
        contact, gap = contact + int((ref["dist"][m] == 0).sum()), gap + int((ref["dist"][m] > 0).sum())
    assert contact > 0 and gap > 0


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_recorded_poses_and_culling_change_no_bit(robot):
    """the device's route -- recorded relative poses, one mesh distance per stencil point, the slot table, the quotients -- equals the
    single pass bit for bit, with the sphere culling and without; the stencil points number 1 + 2 x (evaluated joints)"""
    case = case_of(robot)
    C, P = case["C"], len(case["pairs"])
    for mode in (False, True):
        sample, scale, pose = item_arrays(case, np.random.default_rng(5), C, P, True)
        want = emul_evaluate(case, C, sample, scale, pose, 1e-7, mode, route=0, cull=True)
        for route, cull in ((0, False), (1, True), (1, False)):
            got = emul_evaluate(case, C, sample, scale, pose, 1e-7, mode, route=route, cull=cull)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (route, cull)
        tup = case["tuples"]
        q = case["q"][:P]
        _, grad, ns = emul_items(case["topo"], case["floating"], case["hulls"], case["meshes"], case["pairs"], q, case["rpy"][:P] if case["floating"] else None,
                                 case["bp"][:P] if case["floating"] else None, mode, 1e-7, route=1)
        for k, (a, b) in enumerate(case["pairs"]):
            on = hg.path_dofs(case["topo"], tup[a][0], tup[b][0], mode)
            assert ns[k] == (0 if case["classes"][k] == "plain" else 1 + 2 * int(on.sum()))
            assert np.all(grad[k][~on] == 0.0)


# ---- the gantry: a contact of known slope, and a contact without one ---------------------------------------------------------------------------
def gantry_case(gap):
    """The gantry of tests/hull_shapes.py (DOF 0 lifts along z, DOF 1 slides along x; exact poses).  The bed carries the surface of a slab
    whose top face is z = 0 as a mesh (12 triangles), the carriage a tetrahedron, apex down at its origin, as a mesh (4 triangles) AND as
    a hull; a world box hangs ``gap`` above the tetrahedron's flat top.  The apex is ``gap`` above the slab's top face (negative: through
    it), away from the face's diagonal.  Pairs (bed, carriage), (carriage, bed), (carriage, lid), (lid, carriage): lifting opens the lower
    gap and closes the upper one.  ``meshes_hull``: the carriage as a solid hull, the bed meshed; ``meshes``: both meshed."""
    from flobaroid_amd.collision import Box, Hull, hull_from_box

    topo = hs.gantry()
    slab = box_triangles([0.5, 0.5, 0.0625], [0.0, 0.0, -0.0625])
    tet = np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.125], [-0.0625, 0.125, 0.125], [-0.0625, -0.125, 0.125]])
    faces = np.array([[tet[a], tet[b], tet[c]] for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))])
    hulls = [Hull("bed", slab.reshape(-1, 3), np.zeros(3)), Hull("carriage", tet, np.zeros(3)),
             hull_from_box(Box(None, np.array([0.25, 0.25, 0.125]), np.array([0.125, 0.0, 0.25 + 2.0 * gap]), np.eye(3), "lid"))]
    q = np.array([[-0.5 + gap, -0.125]])  # the apex at (0.125, 0, gap)
    pairs = np.array([[0, 1], [1, 0], [1, 2], [2, 1]], dtype=np.int32)
    return {"robot": "gantry", "topo": topo, "floating": False, "hulls": hulls, "tuples": as_tuples(topo, hulls), "pairs": pairs, "q": q, "rpy": None,
            "bp": None, "C": 1, "meshes": {0: slab, 1: faces}, "meshes_hull": {0: slab}}


STACK_ROWS = thg.STACK_ROWS


@pytest.mark.parametrize("mode", [False, True], ids=["world-axes", "link-axes"])
@pytest.mark.parametrize("which", ["meshes", "meshes_hull"])
def test_gantry_apex_over_a_mesh_face(which, mode):
    """the apex 1e-2 above the face: the distance is the gap, the row +-1 in the lift and 0 in the slide within the bar, in the emulation
    and in the restatement; the apex 1e-3 THROUGH the face: the distance is 0.0 and the row EXACTLY 0.0 -- a mesh has no depth"""
    smp = np.zeros((1, 4), dtype=np.int64)
    for eps in (1e-7, 1e-4):
        case = gantry_case(1e-2)
        meshes = case[which]
        ref, ed, eg = reference(case, 1, case["pairs"], smp, None, None, eps, mode, meshes=meshes)
        assert ref["meshed"].all() if which == "meshes" else list(ref["meshed"]) == [True, True, False, False]
        assert np.all(np.abs(ed[0] - 1e-2) <= ref["dist_bar"][0]) and np.all(np.abs(ref["dist"][0] - 1e-2) <= ref["dist_bar"][0])
        assert np.all(np.abs(eg[0] - STACK_ROWS) <= ref["bar"][0]) and np.all(np.abs(ref["grad"][0] - STACK_ROWS) <= ref["bar"][0])
        assert ref["on_path"][0].all() and np.all(ref["bar"] < 1e-3)
        case = gantry_case(-1e-3)
        ref, ed, eg = reference(case, 1, case["pairs"], smp, None, None, eps, mode, meshes=meshes)
        m = ref["meshed"]
        assert np.all(ref["signed0"][0][m] < -1e-4) and np.all(ed[0][m] == 0.0) and np.all(eg[0][m] == 0.0) and np.all(ref["grad"][0][m] == 0.0)
        # (the plain pairs of the same set keep their depth and their slope)
        assert np.all(np.abs(eg[0][~m] - STACK_ROWS[~m]) <= ref["bar"][0][~m]) and np.all(ed[0][~m] < 0.0)


# ---- the reason for the feature --------------------------------------------------------------------------------------------------------------
def channel_case(C=4):
    """tests/test_meshes.small_mesh_set: the U-channel on the gantry's bed as a mesh, a tetrahedron on the carriage moving inside it"""
    from test_meshes import small_mesh_set

    topo, cfg, cs = small_mesh_set()
    rng = np.random.default_rng(4)
    q = np.stack([rng.uniform(-0.1, 0.1, C), rng.uniform(-0.15, 0.15, C)], axis=1)
    hulls = list(cs["hulls"])
    return {"robot": "gantry", "topo": topo, "floating": False, "hulls": hulls, "tuples": as_tuples(topo, hulls),
            "pairs": np.asarray(cs["hull_pairs"], dtype=np.int32).reshape(-1, 2), "q": q, "rpy": None, "bp": None, "C": C, "meshes": dict(cs["meshes"]),
            "cs": cs, "config": cfg}


def test_tetrahedron_inside_the_u_channel():
    """Inside the channel's hull and clear of its slabs: the mesh row equals the restatement within the bar at a positive distance; the
    hull gradient of the same set without meshes reports a penetration at every placement and, at two of the four at least, a row that
    differs from the mesh row by more than both bars -- the hull pushes the tetrahedron out of a channel it is not touching.
    Measured: mesh distances 0.16 to 0.25, hull distances -0.15 to -0.33, largest |hull row - mesh row| 1.000."""
    case = channel_case()
    C, P = case["C"], len(case["pairs"])
    smp = np.zeros((C, P), dtype=np.int64)
    one = dict(case, q=case["q"])
    # (every candidate is one sample long here)
    ref, ed, eg = reference(one, C, case["pairs"], smp, None, None, 1e-7, False)
    assert ref["meshed"].all() and np.all(ed > 0.01) and np.all(np.abs(eg - ref["grad"]) <= ref["bar"]) and np.all(np.abs(ed - ref["dist"]) <= ref["dist_bar"])
    hd, hgr = thg.emul_evaluate(one, C, smp, None, None, 1e-7, False, case["pairs"])
    href = hg.evaluate(case["topo"], case["tuples"], case["pairs"], False, case["q"], None, None, C, smp, None, None, 1e-7, False)
    href = hg.with_dev(href, float(np.abs(hd - href["dist"]).max()))
    assert np.all(hd < 0.0) and np.all(np.abs(hgr - href["grad"]) <= href["bar"])
    apart = (np.abs(hgr - eg) > ref["bar"] + href["bar"]).any(axis=2)
    print(f"U-channel: mesh distances {ed.reshape(-1)}, hull distances {hd.reshape(-1)}, largest |hull row - mesh row| = {np.abs(hgr - eg).max():.3f}")
    assert apart.sum() >= 2  # (where both rows are the lift alone -- the floor below, the way out above -- they coincide)


# ---- the restatement's own yardstick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["kuka_lwr4", "walkman_left_arm"])
def test_restatement_against_richardson_extrapolation(robot):
    """tests/test_hull_gradient.py's yardstick on the mesh restatement: at eps = 1e-4 against (4 D(h/2) - D(h)) / 3 of central differences D
    of the restated distance at h = 1e-3, on the entries whose three distances at 0, +-h are positive.  A mesh distance is a minimum over
    triangles: where the winning triangle (or its closest feature) changes on the stencil the entry has a kink and is left out by its
    spread |D(h) - D(h/2)| exceeding the bar, ten times the 99th percentile of the spread; at most 5 % (asserted).
    Measured, 73 entries each: kuka_lwr4 0.00 % left out, max |restatement - Richardson| = 1.7e-9 under a bar of 9.4e-7; walkman_left_arm
    0.00 % left out, 4.3e-6 under 5.3e-5."""
    case = case_of(robot)
    C, P = case["C"], len(case["pairs"])
    sample, scale, pose = item_arrays(case, np.random.default_rng(6), C, P, True)
    args = (case["topo"], case["tuples"], case["meshes"], case["pairs"], case["floating"], case["q"], case["rpy"], case["bp"], C, sample, scale, pose)
    ref, _, eg = reference(case, C, case["pairs"], sample, scale, pose, 1e-4, True)
    h = 1e-3
    Dh, Dh2 = mg.evaluate(*args, h, True), mg.evaluate(*args, h / 2, True)
    rich = (4.0 * Dh2["grad"] - Dh["grad"]) / 3.0
    use = hg.separated(Dh) & ref["on_path"]
    spread = np.abs(Dh["grad"] - Dh2["grad"])
    bar = 10.0 * np.percentile(spread[use], 99)
    smooth = use & (spread <= bar)
    err = np.abs(ref["grad"] - rich)[smooth]
    print(f"{robot}: {int(use.sum())} entries, spread 99th percentile {bar / 10:.2e}, max {spread[use].max():.2e}; left out "
          f"{100 * (1 - smooth.sum() / use.sum()):.2f} %; max |restatement - Richardson| = {err.max():.2e}, bar {bar:.2e}")
    assert use.sum() >= 50 and smooth.sum() >= 0.95 * use.sum()
    assert err.max() <= bar
    assert np.all(np.abs(eg - rich)[smooth] <= bar + ref["bar"][smooth])


# ---- the end-to-end case (shared with tests/test_gpu_mesh_gradient.py) ------------------------------------------------------------------------
E2E_STEP = thg.E2E_STEP
E2E_MAX_EXCLUDED = 0.25
E2E_FD_BAR = 5e-8  # ten times what the restatement alone gives (test_end_to_end_seed_with_the_restatement_alone), rounded up
E2E_MESHED = (2, 6)  # the links of kuka_lwr4 served as meshes


def e2e_case(seed=thg.E2E_SEED):
    """tests/test_hull_gradient.e2e_case -- kuka_lwr4 with a box hull on every link and the lifted floor of world_kuka.urdf, 3 candidates of
    60 samples at 20 Hz, transitions on, the same seed -- with two links served as meshes (fullMeshLinks): the four faces of the
    tetrahedron on every second corner of the link's box, which keeps the Qhull restatement of the block, evaluated 2 x 36 times for the
    differences, at about half a minute"""
    from flobaroid_amd.collision import Mesh, collision_set, world_hulls_from_urdf
    from common import GOLDEN

    base = thg.e2e_case(seed)
    topo, names = base["topo"], base["topo"].link_names
    hulls = {h.link_name: h for h in base["cs"]["hulls"] if h.link_name is not None}
    meshes = {}
    for l in E2E_MESHED:
        h = hulls[names[l]]
        p = 0.5 * (h.vertices.max(0) - h.vertices.min(0)) * np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
        meshes[names[l]] = Mesh(names[l], np.array([[p[a], p[b], p[c]] for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))]), h.offset)
    wh = world_hulls_from_urdf(os.path.join(GOLDEN, "urdf", "world_kuka.urdf"), "geometric")
    wh["ground_link"].offset = wh["ground_link"].offset + np.array([0.0, 0.0, 0.25])
    config = dict(base["config"], fullMeshLinks=[names[l] for l in E2E_MESHED])
    cs = collision_set(topo, {}, config, hulls=hulls, world_hulls=wh, meshes=meshes)
    assert len(cs["meshes"]) == 2 and max(len(t) for t in cs["meshes"].values()) <= 12
    return dict(base, cs=cs, config=config)


def restated_rows(case, cons, q, cands, c, eps):
    """tests/test_hull_gradient.restated_rows on the mesh restatement: candidate c's restated grad_q at the evaluation points of ``cons``
    (the reference's pair order) chained in long double: (ref with its bars, rows (P, E), the bound per row and parameter)"""
    import capsule_gradient_restatement as cg

    topo, cs = case["topo"], case["cs"]
    tup = as_tuples(topo, cs["hulls"])
    hp = np.asarray(cs["hull_pairs"]).reshape(-1, 2)[np.asarray(cs["columns"])[:, 1]]
    C = len(cands)
    mode = bool(cs.get("offset_in_link_axes", False))
    pick = lambda k: np.ascontiguousarray(np.asarray(cons[k]))  # noqa: E731
    sub = {"topo": topo, "floating": False, "hulls": cs["hulls"], "tuples": tup, "pairs": hp, "q": q, "rpy": None, "bp": None, "meshes": cs["meshes"]}
    ref, _, _ = reference(sub, C, hp, pick("eval_sample"), pick("eval_scale"), pick("eval_pose"), eps, mode)
    cand = cands[c]
    smp, sc = pick("eval_sample")[c], pick("eval_scale")[c]
    want = cg.position_chain(cand["wf"], cand["q_range"], cand["a"], cand["b"], smp, sc, ref["grad"][c], case["freq"], dtype=np.longdouble).astype(np.float64)
    n = topo.num_dofs
    bound = np.zeros_like(want)
    for d in range(n):  # |d row| <= |scale| sum_d bar[d] |dq_d/dp|, joint by joint
        e = np.zeros((len(smp), n))
        e[:, d] = ref["bar"][c][:, d]
        bound += np.abs(cg.position_chain(cand["wf"], cand["q_range"], cand["a"], cand["b"], smp, sc, e, case["freq"]))
    qr = 1.0 if cand["q_range"] is None else max(1.0, float(np.max(cand["q_range"])))
    bound += (1e-12 * np.abs(sc) * np.abs(ref["grad"][c]).sum(axis=1) * qr)[:, None]
    return ref, want, bound


class HostMeshGradientEngine:
    """tests/test_meshes.HostMeshEngine (candidate_hull_distances from the restatement) with mesh_distance_gradients answered by the
    emulation: what the mesh_gradient=True path of excitation needs of an Engine on the CPU"""

    def __init__(self, topo, floating):
        from test_meshes import HostMeshEngine

        self._values = HostMeshEngine(topo, floating)
        self.topo, self.floating, self.n, self.calls = topo, floating, topo.num_dofs, self._values.calls

    def set_hulls(self, hulls, pairs, offset_in_link_axes=False, meshes=None):
        self._values.set_hulls(hulls, pairs, offset_in_link_axes, meshes)
        self.hulls, self.pairs, self.mode, self.meshes = list(hulls), np.asarray(pairs).reshape(-1, 2), offset_in_link_axes, dict(meshes or {})

    def candidate_hull_distances(self, *a, **k):
        return self._values.candidate_hull_distances(*a, **k)

    def hull_distance_gradients(self, *a, **k):
        raise AssertionError("a set with meshes goes to mesh_distance_gradients")

    def mesh_distance_gradients(self, st, C, sample, scale=None, pose_sample=None, base_pos=None, epsilon=None):
        assert self.meshes, "installed without its meshes"
        self.calls.append(("mesh_gradients", epsilon))
        sub = {"topo": self.topo, "floating": self.floating, "hulls": self.hulls, "pairs": self.pairs, "q": np.asarray(st["q"]), "rpy": st.get("rpy"),
               "bp": base_pos, "meshes": self.meshes}
        d, g = emul_evaluate(sub, C, sample, scale, pose_sample, epsilon, self.mode)
        return {"dist": d, "grad_q": g}

    def fourier_position_chain(self, wf, A, B, sample, grad_q, freq, scale=None, q_range=None):
        import capsule_gradient_restatement as cg

        return np.stack([cg.position_chain(wf[c], None if q_range is None else q_range[c], A[c], B[c], sample[c], None if scale is None else scale[c],
                                           grad_q[c], freq) for c in range(len(wf))])


@functools.lru_cache(maxsize=None)
def e2e_block():
    """(case, candidates, q, engine, the collision block of the restatement) of e2e_case"""
    from flobaroid_amd import excitation as exc

    case = e2e_case()
    cands = [case["make"](x) for x in case["xs"]]
    q = np.concatenate([thg.host_positions(cd, case["T"], case["freq"]) for cd in cands])
    eng = HostMeshGradientEngine(case["topo"], False)
    cons = exc._collision_block(eng, {"q": q}, case["C"], case["config"], case["cs"])
    return case, cands, q, eng, cons


def test_end_to_end_seed_with_the_restatement_alone():
    """The experiment of tests/test_gpu_mesh_gradient.py's end-to-end test without the device: the collision block of one candidate from the
    mesh restatement (HostMeshEngine), differenced over +-1e-6 in every optimiser variable, against the restated central differences at
    eps = 1e-7 chained to the variables.  Gives the bar of the device's comparison (ten times the figure here) and checks that the seed
    leaves out at most a quarter of the rows: those no configuration won, those whose winning configuration changes on the stencil, and
    those whose centre distance is 0 (a mesh pair in contact) or negative (a plain pair).  A change of the winning TRIANGLE is not tracked:
    the meshes are closed convex surfaces, whose distance has their hull's kinks and no others, and no row needed leaving out for it.
    Measured: max |row - FD| = 4.5e-9 over 13 of the 14 rows (7 of the 8 mesh rows; 3 won by a transition configuration), max |row| 0.92:
    E2E_FD_BAR = 5e-8."""
    from flobaroid_amd import excitation as exc

    case, cands, q, eng, cons = e2e_block()
    topo, cs, config, C, Tn, freq = case["topo"], case["cs"], case["config"], case["C"], case["T"], case["freq"]
    P, n = len(cs["pair_names"]), topo.num_dofs
    assert np.all(np.asarray(cs["columns"])[:, 0] == 2) and 6 <= P <= 16
    trans = (cons["idx"] < 0) & (cons["g"] < 1e10)
    c = int(np.argmax(trans.sum(axis=1)))
    assert trans[c].any(), "no transition configuration wins a pair: choose another seed"
    ref, want, _ = restated_rows(case, cons, q, cands, c, 1e-7)
    nh = cands[c]["a"].shape[1]
    rows = exc.constraint_gradient_to_optimizer_variables({k: v for k, v in exc._gradient_dict(want, n, nh).items()}, cands[c], case["nf"])
    margins = np.asarray(cs["margins"], dtype=np.float64)

    def block(x):
        b = exc._collision_block(eng, {"q": thg.host_positions(case["make"](x), Tn, freq)}, 1, config, cs)
        return b["g"][0], b["idx"][0]

    fd, keep = thg.variable_differences(block, case["xs"][c], margins)
    err = np.abs(fd - rows)[keep].max()
    meshed = ref["meshed"]
    print(f"restatement alone: candidate {c}, {int(keep.sum())} of {P} rows kept ({int((keep & meshed).sum())} of {int(meshed.sum())} mesh rows; "
          f"{int(trans[c].sum())} won by a transition configuration), max |row - FD| = {err:.2e}, max |row| = {np.abs(rows[keep]).max():.3f}")
    assert keep.sum() >= (1.0 - E2E_MAX_EXCLUDED) * P, "more than a quarter of the rows are left out: choose another seed"
    assert (keep & meshed).any() and 10.0 * err <= E2E_FD_BAR and np.abs(rows[keep]).max() > 1e-2


# ---- excitation: the rows against a host engine -----------------------------------------------------------------------------------------------
def test_mesh_rows_in_the_reference_order_and_the_refusals():
    """mesh_gradient=True installs the set WITH its meshes, evaluates Engine.mesh_distance_gradients at the evaluation points of the
    constraint block in the set's own pair order and returns the rows in the reference's, for fullMeshLinks and for collisionMode "full";
    without the keyword everything raises what it raised before; the keyword with a set without meshes, or in capsule / box mode, raises"""
    from flobaroid_amd import excitation as exc

    case, cands, q, eng, cons = e2e_block()
    topo, cs, config, C, freq = case["topo"], case["cs"], case["config"], case["C"], case["freq"]
    cols = np.asarray(cs["columns"])
    hp = np.asarray(cs["hull_pairs"]).reshape(-1, 2)[cols[:, 1]]
    # the set's own pair order turned round, the reference's kept: pair k of the reference is pair P - 1 - k of the set
    cs = dict(cs, hull_pairs=np.ascontiguousarray(hp[::-1]), columns=np.stack([np.full(len(hp), 2), np.arange(len(hp))[::-1]], axis=1))
    sub = {"topo": topo, "floating": False, "hulls": cs["hulls"], "pairs": hp, "q": q, "rpy": None, "bp": None, "meshes": cs["meshes"]}
    pick = lambda k: np.ascontiguousarray(np.asarray(cons[k]))  # noqa: E731
    want_d, want_g = emul_evaluate(sub, C, pick("eval_sample"), pick("eval_scale"), pick("eval_pose"), 3e-6, False)
    st = {"q": q}
    for cfg in (dict(config, analyticalGradientEpsilon=3e-6), dict(config, analyticalGradientEpsilon=3e-6, collisionMode="full", fullMeshLinks=[])):
        del eng.calls[:]
        out = exc.candidate_collision_gradient(eng, st, C, cands, freq, cfg, cs, constraints=cons, mesh_gradient=True)
        assert eng.calls == [("set_hulls", sorted(cs["meshes"])), ("mesh_gradients", 3e-6)]
        assert out["grad_q"].tobytes() == want_g.tobytes() and np.array_equal(out["g"], cons["g"])
        won = pick("eval_sample") >= 0
        assert np.abs(want_d - np.asarray(cs["margins"])[None] - cons["g"])[won].max() <= 1e-9  # (the block is the restatement's)
        assert out["grad"]["a"].shape[:3] == (C, len(cols), topo.num_dofs) and np.abs(out["grad"]["q_offset"]).max() > 1e-2
    # the other keywords change nothing beside it; the function's own epsilon wins
    del eng.calls[:]
    exc.candidate_collision_gradient(eng, st, C, cands, freq, config, cs, constraints=cons, mesh_gradient=True, hull_gradient=True, box_gradient=True,
                                     epsilon=1e-5)
    assert eng.calls[-1] == ("mesh_gradients", 1e-5)
    # without the keyword: the refusals of before, by the names of the meshed links
    names = [topo.link_names[l] for l in E2E_MESHED]
    limits = {j: {"lower": -1.0, "upper": 1.0, "velocity": 1.0, "torque": 1.0} for j in topo.dof_names}
    for kw in ({}, {"mesh_gradient": False}, {"hull_gradient": True}, {"box_gradient": True, "hull_gradient": True}):
        with pytest.raises(ValueError, match=r"triangle meshes.*" + names[0]):
            exc.candidate_collision_gradient(eng, st, C, cands, freq, config, cs, constraints=cons, **kw)
        with pytest.raises(ValueError, match=r"triangle meshes.*" + names[0]):
            exc.candidate_gradients_from_coefficients(eng, cands, case["T"], freq, None, None, limits, topo.dof_names, config, collision=cs, **kw)
    # the keyword with what it does not cover
    plain = {k: v for k, v in cs.items() if k != "meshes"}
    convex = {k: v for k, v in config.items() if k != "fullMeshLinks"}
    for fn in (lambda c_, s_: exc.candidate_collision_gradient(eng, st, C, cands, freq, c_, s_, constraints=cons, mesh_gradient=True),
               lambda c_, s_: exc.candidate_gradients_from_coefficients(eng, cands, case["T"], freq, None, None, limits, topo.dof_names, c_, collision=s_,
                                                                        mesh_gradient=True)):
        with pytest.raises(ValueError, match="mesh_gradient=True.*no triangle meshes"):
            fn(config, plain)
        with pytest.raises(ValueError, match="mesh_gradient=True.*no triangle meshes"):
            fn(convex, plain)
        with pytest.raises(ValueError, match="mesh_gradient=True.*without fullMeshLinks"):
            fn(convex, cs)
        for mode in ("capsule", "box"):
            with pytest.raises(ValueError, match=f"mesh_gradient=True.*collisionMode '{mode}'"):
                fn(dict(convex, collisionMode=mode), cs)
            with pytest.raises(ValueError, match=f"mesh_gradient=True.*collisionMode '{mode}'"):
                fn(dict(config, collisionMode=mode), plain)
    with pytest.raises(ValueError, match="suspended"):
        exc.candidate_collision_gradient(eng, st, C, cands, freq, dict(config, floatingBaseAttachment="suspended"), cs, constraints=cons, mesh_gradient=True)


def test_mesh_gradient_symbol_in_header_binding_and_library():
    """added under C-ABI 104: the version stays, header, binding and library carry the symbol, with the hull call's signature"""
    from flobaroid_amd import _lib

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    name = "fbr_mesh_distance_gradients"
    assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr)
    assert _lib._SIGNATURES[name] == _lib._SIGNATURES["fbr_hull_distance_gradients"]
    assert lib.fbr_version() == _lib.FBR_VERSION == 104 == int(re.search(r"#define FBR_VERSION (\d+)", hdr).group(1))
    assert hasattr(_lib.Engine, "mesh_distance_gradients")
    api = open(os.path.join(ROOT, "flobaroid_amd", "csrc", "fbr_api.hip")).read()
    assert name + ": added symbols" in api and name in hdr.split("#define FBR_VERSION")[0]  # (the lists of symbols added under 104)
    assert hr.EPS == mg.EPS == mr.EPS
