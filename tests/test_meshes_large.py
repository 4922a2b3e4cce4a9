"""Meshes of up to FBR_MAX_LARGE_MESH_TRIANGLES triangles behind a tree, off the GPU: the HIP-free text of csrc/fbr_mesh_bvh.h (g++,
tests/emul/mesh_bvh_emul.cpp) -- the builder, the checks of fbr_model_set_large_hull_meshes, and the traversal walked as a wave walks it,
over packets of up to 64 poses at once -- against the brute force of csrc/fbr_mesh.h with its culling off on the same poses (the SAME
BITS: a strict minimum of the same values in another order) and, on a subsample, against the restatement of tests/mesh_restatement.py; the
host side (collision_set(..., large_meshes=), Engine.set_hulls(..., large_meshes=), the gradient refusals of flobaroid_amd/excitation.py)
and the new symbol.  Needs no GPU.

The comparison with the restatement keeps the rule of tests/test_meshes.py: first the restatement's signed value is more than 100 bars from
0 (a bar: 32 eps x the pair's scale), then the assertion is the bar; no case is dropped, the seeds are such that every case is clear.

Measured here (g++, -ffp-contract=off): brute emulation against the restatement 0.98 eps x scale at most (blob x blob, torus x sheet,
torus x prism, sheet x box, soup x sheet, box x torus: 19 poses apart, 3 intersecting).  The tree evaluates 0.09 % (soup of 257 x torus)
to 1.3 % (blob x blob) of the triangle pairs of two meshes in the random poses, 8 % to 26 % of a mesh's triangles against a solid (the
sheet against a box is the worst: a sphere bounds a thin triangle badly), and 44 % of the 8 x 9 soups, whose trees are one and three nodes.
KUKA's link_7 x link_6 (2 024 712 triangle pairs): 37 081 = 1.83 % with the flange 0.11 m above the wrist, face to face, through 6556 node
pairs; 23 evaluations when the two interlock (the first leaf pair touches: 0.0 ends the lane).  Deepest tree here 8 levels, highest stack
16 of 64 pairs, at most 10 GJK iterations."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hull_restatement as hr
import hull_shapes as hs
import mesh_large_shapes as ml
import mesh_restatement as mr
import test_meshes as tm
from common import GOLDEN, ROOT
from test_boxes import random_rotations
from test_hulls import _c, _p, tables

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "mesh_bvh_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libmesh_bvh_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_lib = None
EPS = np.finfo(np.float64).eps
BAR = 32.0  # x eps x scale, as tests/test_meshes.py
URDF = os.path.join(GOLDEN, "urdf")
STATS = ("node_pairs", "leaf_pairs", "tri_pairs", "evals", "max_stack", "max_iter", "max_depth", "all_pairs")


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC, os.path.join(ROOT, "include", "fbr.h")] + [os.path.join(_CSRC, h) for h in ("fbr_mesh_bvh.h", "fbr_mesh.h", "fbr_hull.h", "fbr_box.h",
                                                                                                   "fbr_capsule.h", "fbr_math.h", "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


def leaf():
    return int(emul().bvh_leaf())


def build(tris):
    """(node (N, 4), vol (N, 4), depth (N,), order (T,)) of the tree of tris (T, 3, 3)"""
    t = _c(np.asarray(tris).reshape(-1, 9))
    cap = 2 * len(t) + 2
    node, vol, depth, order = np.zeros((cap, 4), dtype=np.int32), np.zeros((cap, 4)), np.zeros(cap, dtype=np.int32), np.zeros(len(t), dtype=np.int32)
    msg = ctypes.create_string_buffer(256)
    n = emul().bvh_build(ctypes.c_long(len(t)), _p(t), cap, _p(node), _p(vol), _p(depth), _p(order), msg, 256)
    assert n > 0, msg.value.decode()
    return node[:n], vol[:n], depth[:n], order


def pairs_emul(fr, hulls, meshes, pairs, tree, packet=64):
    """(dist (S, P), stats {name: value}) of the frames fr (S, H, 12): tree False the brute force without culling, True the tree walked over
    packets of ``packet`` consecutive poses"""
    vbeg, v, fbeg, pl, ebeg, ed, diam = tables(hulls)
    mtab, tris = tm.mesh_tables(len(hulls), meshes)
    fr, pr = _c(fr), _c(pairs, np.int32).reshape(-1, 2)
    S, P = fr.shape[0], len(pr)
    dist, stats = np.zeros((S, P)), np.zeros(8, dtype=np.int64)
    emul().bvh_pairs(ctypes.c_long(S), len(hulls), _p(fr), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), _p(diam), _p(mtab), _p(tris),
                     ctypes.c_long(len(tris)), P, _p(pr), int(tree), int(packet), _p(dist), stats.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return dist, dict(zip(STATS, (int(x) for x in stats)))


def same_bits(fr, hulls, meshes, pairs, why, packet=64):
    """the tree's values, asserted to be the brute force's bit for bit (a NaN by its place); also (tree stats, brute stats)"""
    a, sa = pairs_emul(fr, hulls, meshes, pairs, True, packet)
    b, sb = pairs_emul(fr, hulls, meshes, pairs, False)
    assert a.tobytes() == b.tobytes() or (np.array_equal(np.isnan(a), np.isnan(b)) and a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()), why
    assert sa["max_stack"] <= int(emul().bvh_stack()) and sa["max_depth"] <= int(emul().bvh_max_depth())
    assert 4 * max(sa["max_iter"], sb["max_iter"]) < tm.MAX_ITER
    return a, sa, sb


# ---- the shapes ----------------------------------------------------------------------------------------------------------------------------------
def shapes():
    L = leaf()
    return {"torus": ml.torus(), "sphere": ml.sphere(), "sheet": ml.sheet(), "blob": ml.blob(3), "blob2": ml.blob(4), "soupL": ml.soup(1, L),
            "soupL1": ml.soup(2, L + 1), "soup2L1": ml.soup(3, 2 * L + 1), "soup257": ml.soup(4, 257)}


def test_shapes_have_the_counts_the_caps_are_about():
    from flobaroid_amd.collision import FBR_MAX_HULL_VERTICES, FBR_MAX_MESH_PAIR_WORK, FBR_MAX_MESH_TRIANGLES

    s = shapes()
    assert {k: len(v) for k, v in s.items() if not k.startswith("soup")} == {"torus": 640, "sphere": 260, "sheet": 512, "blob": 182, "blob2": 182}
    assert len(ml.hull_of(s["sphere"], "a", pad=None).vertices) == 132 > FBR_MAX_HULL_VERTICES
    assert 182 < FBR_MAX_MESH_TRIANGLES < 257 and 182 * 182 > FBR_MAX_MESH_PAIR_WORK
    assert len(ml.hull_of(s["torus"], "a").vertices) == 8


# ---- 1. the builder ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["torus", "sphere", "sheet", "blob", "soupL", "soupL1", "soup2L1", "soup257"])
def test_builder(kind):
    t = shapes()[kind]
    L, T = leaf(), len(t)
    node, vol, depth, order = build(t)
    again = build(t)
    assert all(np.array_equal(x, y) for x, y in zip((node, vol, depth, order), again)), "the builder is deterministic"
    assert np.array_equal(np.sort(order), np.arange(T))  # a permutation
    leaves = node[:, 0] < 0
    assert np.all((node[leaves, 1] < 0) & (node[leaves, 3] <= L) & (node[leaves, 3] >= 1))
    # every triangle in exactly one leaf: the leaves' ranges tile [0, T)
    cover = np.zeros(T, dtype=np.int64)
    for f, n in node[leaves][:, 2:]:
        cover[f:f + n] += 1
    assert np.all(cover == 1)
    sorted_t = t.reshape(-1, 9)[order].reshape(-1, 3, 3)
    for i, (l, r, f, n) in enumerate(node):
        if l >= 0:  # the children halve the range, one level down
            assert tuple(node[l, 2:]) == (f, n // 2) and tuple(node[r, 2:]) == (f + n // 2, n - n // 2) and n > L
            assert depth[l] == depth[r] == depth[i] + 1
        pts = sorted_t[f:f + n].reshape(-1, 3)
        assert np.all(np.linalg.norm(pts - vol[i, :3], axis=1) <= vol[i, 3]), "a node's sphere holds the vertices of its triangles"
    assert node[0, 2] == 0 and node[0, 3] == T and depth[0] == 0
    want_depth = 0 if T <= L else int(np.ceil(np.log2(T / L)))
    assert depth.max() == want_depth <= int(emul().bvh_max_depth())
    assert int(emul().bvh_stack()) >= 2 * int(emul().bvh_max_depth()) + 2
    if kind in ("soupL", "soupL1", "soup2L1"):
        assert len(node) == {"soupL": 1, "soupL1": 3, "soup2L1": 5}[kind]


def _validate(hulls, link, pairs, meshes, edit=None):
    """the checks of fbr_model_set_large_hull_meshes (the same text): (0 or -1, message); meshes: [(hull, triangles)]"""
    _, _, fbeg, pl, _, _, diam = tables(hulls) if hulls else (None, None, _c([0], np.int32), np.zeros((0, 4)), None, None, np.zeros(0))
    arr = {"hull": _c([h for h, _ in meshes], np.int32), "tbeg": _c(np.cumsum([0] + [len(t) for _, t in meshes]), np.int32),
           "tris": _c(np.concatenate([np.asarray(t).reshape(-1, 9) for _, t in meshes]) if meshes else np.zeros((0, 9)))}
    if edit:
        edit(arr)
    link, pr = _c(link, np.int32), _c(pairs, np.int32).reshape(-1, 2)
    msg = ctypes.create_string_buffer(256)
    rc = emul().bvh_validate(len(hulls), _p(link), _p(fbeg), _p(pl), _p(diam), len(pr), _p(pr), len(meshes), _p(arr["hull"]), _p(arr["tbeg"]),
                             _p(arr["tris"]), msg, 256)
    return rc, msg.value.decode()


def test_large_meshes_are_refused_as_the_header_lists():
    """every message of fbr_mesh_validate with the large caps, the 8193-triangle refusal, and what the small call refuses and this one takes"""
    rng = np.random.default_rng(6)
    soups = [tm._soup(rng, n, 0.2) for n in (5, 9, 3, 4)]
    hulls, tris = [h for _, h in soups], [t for t, _ in soups]
    link, pairs = [0, 2, 1, -1], [[0, 1], [0, 3], [1, 2]]
    ok = [(0, tris[0]), (1, tris[1])]
    assert _validate(hulls, link, pairs, ok) == (0, "") and _validate(hulls, link, pairs, []) == (0, "")

    def put(key, index, value):
        def edit(arr):
            arr[key].reshape(-1)[index] = value
        return edit

    rep = lambda t, n: np.tile(t[:1], (n, 1, 1))  # noqa: E731
    bad = {
        "no hull set": dict(hulls=[], link=[], pairs=[], meshes=[]), "out of range": dict(meshes=[(4, tris[0])]), "out of range ": dict(meshes=[(-1, tris[0])]),
        "given twice": dict(meshes=[(0, tris[0]), (0, tris[0])]), "world hull": dict(meshes=[(3, tris[3])]),
        "tbeg starts at 0": dict(meshes=ok, edit=put("tbeg", 0, 1)), "not ascending": dict(meshes=ok, edit=put("tbeg", 2, 3)),
        "no triangle": dict(meshes=[(0, tris[0]), (1, np.zeros((0, 3, 3)))]), "non-finite": dict(meshes=ok, edit=put("tris", 7, np.nan)),
        "outside face": dict(meshes=[(0, tris[0] * 3.0)]), "8193 triangles on hull 0, more than 8192": dict(meshes=[(0, rep(tris[0], 8193))]),
    }
    for why, kw in bad.items():
        rc, msg = _validate(kw.get("hulls", hulls), kw.get("link", link), kw.get("pairs", pairs), kw["meshes"], kw.get("edit"))
        assert rc == -1 and why.strip() in msg, (why, msg)
    # what fbr_model_set_hull_meshes refuses by count: 257 triangles, 182 x 182 triangle pairs, and the cap itself
    assert tm._validate(hulls, link, pairs, [(0, rep(tris[0], 257))])[0] == -1 and _validate(hulls, link, pairs, [(0, rep(tris[0], 257))]) == (0, "")
    both182 = [(0, rep(tris[0], 182)), (1, rep(tris[1], 182))]
    assert tm._validate(hulls, link, pairs, both182)[0] == -1 and _validate(hulls, link, pairs, both182) == (0, "")
    assert _validate(hulls, link, pairs, [(0, rep(tris[0], 8192))]) == (0, "")  # (identical triangles: the median split still halves)


# ---- 2. the tree against the brute force: the same bits -------------------------------------------------------------------------------------------
def random_frames(rng, S, spread, nh=2):
    """(S, nh, 12): hull 0 near the origin, the others ``spread`` away on average, random rotations; consecutive poses are close to each
    other, as consecutive samples of a trajectory are"""
    R0, c0 = random_rotations(rng, nh), rng.standard_normal((nh, 3)) * spread
    c0[0] *= 0.1
    fr = np.zeros((S, nh, 12))
    w = rng.standard_normal((nh, 3)) * 0.4
    for s in range(S):
        for h in range(nh):
            a = w[h] * (s / 64.0)
            K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
            th = np.linalg.norm(a)
            Rs = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th**2) * K @ K if th > 0 else np.eye(3)
            fr[s, h, :9] = (Rs @ R0[h]).reshape(9)
            fr[s, h, 9:] = c0[h] * (1.0 + 0.3 * s / 64.0)
    return fr


CASES = {  # kind of A, kind of B (None: a solid), the solid, poses, spread
    "torus x sheet": ("torus", "sheet", None, 12, 0.7), "blob x blob (182 x 182)": ("blob", "blob2", None, 67, 0.25),
    "soup257 x torus": ("soup257", "torus", None, 20, 0.3), "soupL x soupL1": ("soupL", "soupL1", None, 67, 0.2),
    "soup2L1 x sheet": ("soup2L1", "sheet", None, 67, 0.3), "torus x prism128": ("torus", None, "prism128", 67, 0.4),
    "sheet x box": ("sheet", None, "box", 67, 0.4), "sphere on its large hull x sheet": ("sphere", "sheet", None, 12, 0.3),
    "sphere on its large hull x sphere129": ("sphere", None, "sphere129", 67, 0.5), "box x torus (the mesh second)": (None, "torus", "box", 67, 0.4),
}


def case_geometry(name, rng):
    import hull_large_shapes as hl

    ka, kb, solid, S, spread = CASES[name]
    s = shapes()
    hulls, meshes = [], {}
    for i, k in enumerate((ka, kb)):
        if k is None:
            hulls.append(hl.shape(solid, "b") if solid == "sphere129" else hs.zoo(rng, "b", solid))
        else:
            hulls.append(ml.hull_of(s[k], "ab"[i], pad=None if k == "sphere" else 0.05))
            meshes[i] = s[k]
    return hulls, meshes, S, spread


@pytest.mark.parametrize("name", list(CASES))
def test_tree_gives_the_bits_of_the_brute_force(name):
    rng = np.random.default_rng(list(CASES).index(name) + 20)
    hulls, meshes, S, spread = case_geometry(name, rng)
    fr = random_frames(rng, S, spread)
    got, sa, sb = same_bits(fr, hulls, meshes, [[0, 1]], name)
    share = sa["evals"] / max(sb["evals"], 1)
    print(f"{name}: {S} poses, {int((got == 0).sum())} touching; the tree evaluated {share:.3%} of {sb['evals']} triangle pairs, {sa['node_pairs']} node pairs, "
          f"depth {sa['max_depth']}, stack {sa['max_stack']}, most GJK iterations {max(sa['max_iter'], sb['max_iter'])}")
    assert np.all(got >= 0.0) and sa["evals"] <= sb["evals"]
    # packets of another length walk another way and give the same bits
    assert pairs_emul(fr, hulls, meshes, [[0, 1]], True, 7)[0].tobytes() == got.tobytes()


def test_a_nan_pose_in_one_lane_and_a_lane_that_touches_early():
    rng = np.random.default_rng(11)
    s = shapes()
    hulls, meshes = [ml.hull_of(s["blob"], "a"), ml.hull_of(s["blob2"], "b")], {0: s["blob"], 1: s["blob2"]}
    fr = random_frames(rng, 64, 0.6)
    fr[5, 1, 10] = np.nan      # a dead lane
    fr[9, 1, 9:] = fr[9, 0, 9:]  # the two blobs on top of each other: 0.0 after a few leaf pairs
    got, sa, sb = same_bits(fr, hulls, meshes, [[0, 1]], "nan / touch")
    assert np.isnan(got[5, 0]) and got[9, 0] == 0.0 and np.isfinite(np.delete(got[:, 0], 5)).all() and (np.delete(got[:, 0], [5, 9]) > 0).all()
    fr[:, 1, 9:] = np.nan  # every lane dead: nothing is evaluated
    got, sa, _ = same_bits(fr, hulls, meshes, [[0, 1]], "all nan")
    assert np.isnan(got).all() and sa["evals"] == 0


@pytest.mark.parametrize("kind", list(tm.contact_kinds()))
def test_exact_contacts_inside_a_tree(kind):
    """the contacts of tests/test_meshes.py at the gaps 1e-9, 0, -1e-9 -> the gap, 0.0, 0.0: the touching triangles are one of 2 L + 1 of
    each mesh, the others 8 m away on the far side, so the contact sits in a leaf two levels down; one packet holds the three gaps"""
    triA, fB = tm.contact_kinds()[kind]
    L = leaf()
    far = ml.soup(9, 2 * L, 0.2)
    gaps = (1e-9, 0.0, -1e-9)
    for R, c in ((np.eye(3), np.zeros(3)), (hs.TURNS["on_side"], np.array([0.5, -0.25, 2.0]))):
        for gap in gaps:
            tA = np.concatenate([triA[None], far - np.array([0.0, 0.0, 8.0])])
            tB = np.concatenate([far + np.array([0.0, 0.0, 8.0]), fB(gap)[None]])
            A, B = tm.solid("a", tA), tm.solid("b", tB)
            fr = tm.frames(np.stack([R, R])[None], np.stack([c, c])[None])
            got, sa, _ = same_bits(fr, [A, B], {0: tA, 1: tB}, [[0, 1]], (kind, gap))
            scale = hr.pair_scale(c, A.diameter, c, B.diameter)
            assert sa["max_depth"] == 2
            if gap > 0:
                assert abs(got[0, 0] - gap) <= BAR * EPS * scale, (kind, gap, got)
            else:
                assert got[0, 0] == 0.0, (kind, gap, got)


def test_builder_and_traversal_under_the_sanitizers(tmp_path):
    """tests/emul/mesh_bvh_sanitize.cpp, a program of its own, built with -fsanitize=address,undefined and run here on the CPU"""
    exe = str(tmp_path / "mesh_bvh_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(_HERE, "emul", "mesh_bvh_sanitize.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and not run.stderr, (run.stdout, run.stderr)


# ---- 3. the brute force against the restatement -----------------------------------------------------------------------------------------------------
RESTATED = {"blob x blob (182 x 182)": 6, "torus x sheet": 2, "torus x prism128": 2, "sheet x box": 2, "soup2L1 x sheet": 6, "box x torus (the mesh second)": 4}


def test_brute_force_against_the_restatement():
    worst, nsep, nhit = 0.0, 0, 0
    for name, n in RESTATED.items():
        rng = np.random.default_rng(list(CASES).index(name) + 20)
        hulls, meshes, S, spread = case_geometry(name, rng)
        fr = random_frames(rng, S, spread)[:: max(S // n, 1)][:n]
        got, _ = pairs_emul(fr, hulls, meshes, [[0, 1]], False)
        for s in range(len(fr)):
            RA, cA, RB, cB = fr[s, 0, :9].reshape(3, 3), fr[s, 0, 9:], fr[s, 1, :9].reshape(3, 3), fr[s, 1, 9:]
            signed = mr.mesh_signed(RA, cA, meshes.get(0), hulls[0].vertices, RB, cB, meshes.get(1), hulls[1].vertices)
            scale = hr.pair_scale(cA, hulls[0].diameter, cB, hulls[1].diameter)
            bar = BAR * EPS * scale
            assert abs(signed) > 100.0 * bar, (name, s, signed, "grey zone: change the seed")
            if signed < 0:
                assert got[s, 0] == 0.0, (name, s, signed, got[s, 0])
                nhit += 1
            else:
                assert abs(got[s, 0] - signed) <= bar, (name, s, signed, got[s, 0])
                worst, nsep = max(worst, abs(got[s, 0] - signed) / (EPS * scale)), nsep + 1
    print(f"brute emulation - restatement: {worst:.3g} eps x scale at most; {nsep} poses apart, {nhit} intersecting")
    assert nsep >= 4 and nhit >= 2


# ---- 4. KUKA's real meshes ----------------------------------------------------------------------------------------------------------------------------
def kuka_meshes(links=("lwr_7_link", "lwr_6_link")):
    from flobaroid_amd.collision import FBR_MAX_LARGE_MESH_TRIANGLES, meshes_from_urdf

    return meshes_from_urdf(os.path.join(URDF, "kuka_lwr4.urdf"), list(links), max_triangles=FBR_MAX_LARGE_MESH_TRIANGLES)


def test_kuka_link_7_against_link_6():
    """two (pair, pose) picks of the real meshes, 1098 x 1844 triangles: apart as in the arm (0.078 m between the link origins along z), and
    pushed into each other's bounding boxes"""
    ms = kuka_meshes()
    a, b = ms["lwr_7_link"], ms["lwr_6_link"]
    assert (len(a.triangles), len(b.triangles)) == (1098, 1844) and len(a.hull.vertices) == 158 and len(b.hull.vertices) == 793
    fr = np.zeros((2, 2, 12))
    fr[:, :, :9] = np.eye(3).reshape(9)
    fr[0, 0, 9:], fr[0, 1, 9:] = a.offset + np.array([0.0, 0.0, 0.078 + 0.12]), b.offset
    fr[1, 0, :9] = hs.TURNS["quarter"].reshape(9)
    fr[1, 0, 9:], fr[1, 1, 9:] = a.offset + np.array([0.0, 0.05, 0.078]), b.offset
    shares = []
    for s in range(2):
        got, sa, sb = same_bits(fr[s:s + 1], [a.hull, b.hull], {0: a.triangles, 1: b.triangles}, [[0, 1]], ("kuka", s))
        share = sa["evals"] / sb["all_pairs"]
        shares.append(share)
        print(f"KUKA link_7 x link_6, pose {s}: distance {got[0, 0]:.6g}; the tree evaluated {sa['evals']} of {sb['all_pairs']} triangle pairs = {share:.4%} "
              f"({sa['node_pairs']} node pairs, {sa['leaf_pairs']} leaf pairs holding {sa['tri_pairs']}); depth {sa['max_depth']}, stack {sa['max_stack']}")
        assert sb["all_pairs"] == 1098 * 1844 and got[0, 0] >= 0.0
    # (the bound: DESIGN.md measures the brute-force kernel at 23 x the convex call on pairs of 1e4 triangle pairs; this pair has 2e6, and a
    # tree that left more than a twentieth of them would leave KUKA's "full" mode a thousand convex calls away)
    assert max(shares) < 0.05


# ---- 5. the host side -----------------------------------------------------------------------------------------------------------------------------------
def kuka_full_set(large_meshes=True):
    from flobaroid_amd.collision import FBR_MAX_LARGE_HULL_VERTICES, FBR_MAX_LARGE_MESH_TRIANGLES, collision_set, hulls_from_urdf, meshes_from_urdf
    from common import load_topo

    topo = load_topo("kuka_lwr4")
    urdf = os.path.join(URDF, "kuka_lwr4.urdf")
    hulls, box_links = hulls_from_urdf(urdf, topo.link_names, max_vertices=FBR_MAX_LARGE_HULL_VERTICES)
    ms = meshes_from_urdf(urdf, [n for n in topo.link_names if n in hulls and n not in box_links], max_triangles=FBR_MAX_LARGE_MESH_TRIANGLES)
    return topo, hulls, ms, lambda **kw: collision_set(topo, {}, {"collisionMode": "full"}, hulls=hulls, meshes=ms, **kw)


def test_collision_set_with_and_without_large_meshes():
    from flobaroid_amd import collision

    topo, hulls, ms, make = kuka_full_set()
    assert {n: len(m.triangles) for n, m in ms.items()} == {"lwr_base_link": 4434, "lwr_1_link": 3066, "lwr_2_link": 3134, "lwr_3_link": 3066,
                                                           "lwr_4_link": 3134, "lwr_5_link": 3328, "lwr_6_link": 1844, "lwr_7_link": 1098}
    with pytest.raises(ValueError, match=r"lwr_base_link: 4434 triangles, more than 256"):
        make()
    cs = make(large_meshes=True)
    assert cs["large_meshes"] is True and len(cs["meshes"]) == 8 and len(cs["pair_names"]) == len(cs["hull_pairs"]) > 0
    names = [h.link_name for h in cs["hulls"]]
    assert all(np.array_equal(t, ms[names[h]].triangles) for h, t in cs["meshes"].items())
    # a small set: the keyword lifts the pair cap and nothing else; without it every refusal stays
    s = shapes()
    g = hs.gantry()
    from flobaroid_amd.collision import Mesh

    small = {"bed": Mesh("bed", s["blob"], np.zeros(3)), "carriage": Mesh("carriage", s["blob2"], np.zeros(3))}
    hl = {n: m.hull for n, m in small.items()}
    cfg = {"collisionMode": "full"}
    with pytest.raises(ValueError, match=r"182 x 182 triangle pairs, more than 32768"):
        collision.collision_set(g, {}, cfg, hulls=hl, meshes=small)
    got = collision.collision_set(g, {}, cfg, hulls=hl, meshes=small, large_meshes=True)
    assert got["large_meshes"] is True and sorted(got["meshes"]) == [0, 1]
    one = collision.collision_set(g, {}, {"collisionMode": "convex", "fullMeshLinks": ["bed"]}, hulls=hl, meshes=small)
    assert "large_meshes" not in one
    with pytest.raises(ValueError, match="more than 8192"):
        collision.collision_set(g, {}, cfg, hulls=hl, meshes={"bed": Mesh("bed", np.tile(s["blob"][:1], (8193, 1, 1)) + np.arange(8193)[:, None, None] * 1e-4, np.zeros(3))},
                                large_meshes=True)
    assert collision.FBR_MAX_LARGE_MESH_TRIANGLES == 8192


class RecordingEngine:
    """what excitation._collision_block needs of an Engine, recording the keywords of set_hulls"""

    def __init__(self, topo):
        self.topo, self.n, self.floating, self.calls = topo, topo.num_dofs, False, []

    def set_hulls(self, hulls, pairs, offset_in_link_axes=False, **kw):
        self.calls.append(kw)
        self.P = len(pairs)

    def candidate_hull_distances(self, st, ncand, step=3, base_pos=None, device_out=None):
        return {"dist": np.full((ncand, self.P), 0.5), "idx": np.zeros((ncand, self.P), dtype=np.int64)}


def test_the_collision_block_installs_large_meshes_and_the_gradients_refuse_them():
    from flobaroid_amd import excitation as exc

    topo, hulls, ms, make = kuka_full_set()
    cs = make(large_meshes=True)
    C, T = 2, 6
    q = np.zeros((C * T, topo.num_dofs))
    st = {"q": q, "dq": q.copy(), "ddq": q.copy()}
    config = {"collisionMode": "full", "collisionCheckStep": 1, "transitionDuration": 0.0}
    eng = RecordingEngine(topo)
    blk = exc._collision_block(eng, st, C, config, cs)
    assert blk["g"].shape == (C, len(cs["pair_names"]))
    assert set(eng.calls[0]) == {"meshes", "large", "large_meshes"} and eng.calls[0]["large"] is True and eng.calls[0]["large_meshes"] is True
    # a small set with the keyword: large_meshes without large
    s = shapes()
    from flobaroid_amd.collision import Mesh, collision_set

    g = hs.gantry()
    small = {"bed": Mesh("bed", s["blob"], np.zeros(3)), "carriage": Mesh("carriage", s["soup257"], np.zeros(3))}
    cs2 = collision_set(g, {}, {"collisionMode": "full"}, hulls={n: m.hull for n, m in small.items()}, meshes=small, large_meshes=True)
    eng2 = RecordingEngine(g)
    q2 = np.zeros((C * T, 2))
    exc._collision_block(eng2, {"q": q2, "dq": q2, "ddq": q2}, C, config, cs2)
    assert set(eng2.calls[0]) == {"meshes", "large_meshes"}
    # the gradient entry points, whatever the keywords: by name and count
    limits = {j: {"lower": -1.0, "upper": 1.0, "velocity": 1.0, "torque": 1.0} for j in topo.dof_names}
    for kw in ({}, {"mesh_gradient": True}, {"hull_gradient": True}, {"large_hull_gradient": True}):
        with pytest.raises(ValueError, match=r"lwr_base_link \(4434 triangles on a hull of 216 vertices\).*lwr_7_link \(1098 triangles on a hull of 158"):
            exc.candidate_collision_gradient(eng, st, C, [], 50.0, config, cs, **kw)
        with pytest.raises(ValueError, match=r"large_meshes=True.*lwr_6_link \(1844 triangles on a hull of 793 vertices\)"):
            exc.candidate_gradients_from_coefficients(eng, [], T, 50.0, None, None, limits, topo.dof_names, config, collision=cs, **kw)
    lim2 = {j: {"lower": -1.0, "upper": 1.0, "velocity": 1.0, "torque": 1.0} for j in g.dof_names}
    for kw in ({}, {"mesh_gradient": True}):
        with pytest.raises(ValueError, match=r"carriage \(257 triangles on a hull of \d+ vertices\)"):
            exc.candidate_gradients_from_coefficients(eng2, [], T, 50.0, None, None, lim2, g.dof_names, config, collision=cs2, **kw)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            return 0
        return f


def test_set_hulls_combinations():
    """Engine.set_hulls on a library that records the entry points: which setter runs for which keywords"""
    from flobaroid_amd._lib import Engine

    s = shapes()
    hl = [ml.hull_of(s["blob"], "bed"), ml.hull_of(s["sphere"], "carriage", pad=None)]
    meshes = {0: s["blob"]}

    def run(**kw):
        eng = Engine.__new__(Engine)
        eng.topo, eng._lib, eng._h = hs.gantry(), _Recorder(), None
        eng.set_hulls(hl, [[0, 1]], **kw)
        return eng._lib.calls, eng.num_hull_meshes

    assert run() == (["fbr_model_set_hulls"], 0)
    assert run(meshes=meshes) == (["fbr_model_set_hulls", "fbr_model_set_hull_meshes"], 1)
    assert run(meshes=meshes, large_meshes=True) == (["fbr_model_set_hulls", "fbr_model_set_large_hull_meshes"], 1)
    assert run(meshes=meshes, large=True, large_meshes=True) == (["fbr_model_set_large_hulls", "fbr_model_set_large_hull_meshes"], 1)
    assert run(large=True, large_meshes=True) == (["fbr_model_set_large_hulls"], 0)
    with pytest.raises(ValueError, match=r"set_hulls\(large=True\): triangle meshes on a set of large hulls are not built"):
        run(meshes=meshes, large=True)


def test_large_mesh_symbol_in_header_binding_and_library():
    from flobaroid_amd import _lib, collision

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    name = "fbr_model_set_large_hull_meshes"
    assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr)
    cap = int(re.search(r"#define FBR_MAX_LARGE_MESH_TRIANGLES (\d+)", hdr).group(1))
    assert cap == collision.FBR_MAX_LARGE_MESH_TRIANGLES == _lib.FBR_MAX_LARGE_MESH_TRIANGLES == 8192
    assert hasattr(_lib.Engine, "set_large_hull_meshes") and int(re.search(r"#define FBR_VERSION (\d+)", hdr).group(1)) == lib.fbr_version()
    assert lib.fbr_model_set_large_hull_meshes(None, 0, None, None, None) == -1  # FBR_E_INVALID: no model
    # the shared text: one validation routine, one triangle-range body
    mesh_h = open(os.path.join(_CSRC, "fbr_mesh.h")).read()
    bvh_h = open(os.path.join(_CSRC, "fbr_mesh_bvh.h")).read()
    assert "fbr_mesh_validate" not in bvh_h.split("#pragma once")[1].split("inline std::string fbr_mesh_bvh_build")[0]
    assert mesh_h.count("fbr_hull_gjk(") == 1 and "fbr_hull_gjk(" not in bvh_h and "fbr_mesh_range_oriented<true>" in bvh_h
