"""The gradient of triangle meshes behind a tree off the GPU (csrc/fbr_mesh_bvh_grad.h, fbr_large_mesh_distance_gradients).  Needs no GPU.

* (a) the restatement of the device's three stages (tests/emul/mesh_bvh_grad_emul.cpp route 1: recorded poses, one walk through the trees
  per pose, the quotients) and the stages as the waves run them (routes 2 and 3: packets of 64 consecutive entries, candidate-major and
  slot-major) against the single pass (route 0: fbr_rigidgrad_item with the brute-force fbr_mesh_distance, no culling, as its functor): the
  bytes of dist and grad.  The shapes of tests/mesh_large_shapes.py on KUKA's chain, the first on lwr_2_link, the second on lwr_5_link --
  three revolute joints between them, two above both --, a world box on a vertex of the first mesh at the first configuration (a touching
  centre: distance 0.0 and an exactly zero row) and one far away; every pair in both orders of its members; one NaN joint.
* (b) the entry mapping of both orders is a bijection at S of 1, 3, 63, 64, 65 and C of 1 and 65, and the tiles the kernel cuts a pair into
  (fbr_mesh_bvh_grad_tile) keep every lane's entry inside the pair and store every entry once.
* (c) tests/emul/mesh_bvh_grad_sanitize.cpp under AddressSanitizer and UBSan, a program of its own.
* (d) excitation's large_mesh_gradient keyword against a stub engine: the route, every raise by message, the refusals of before word for word.
* (e) the symbol, the version and the option in header, binding, library and fbr_options.h.

Measured here (g++ 13, x86-64): (a) the bytes equal in all cases; the walks of route 1 evaluate 1 to 15 % of the triangle pairs the
single pass evaluates."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hull_large_shapes as hl
import hull_restatement as hr
import hull_shapes as hs
import mesh_large_shapes as ml
import test_meshes as tm
import test_meshes_large as tl
from common import ROOT, load_topo
from test_hulls import _c, _p, as_tuples, link_index, tables

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "mesh_bvh_grad_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libmesh_bvh_grad_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_lib = None
NONE = 1e10  # FBR_CAPSULE_NONE: the distance of an entry without a sample
STATS = ("node_pairs", "leaf_pairs", "tri_pairs", "evals", "walks", "max_stack")
CANDIDATE_MAJOR, SLOT_MAJOR = 1, 2


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC, os.path.join(ROOT, "include", "fbr.h")] + [os.path.join(_CSRC, h) for h in (
            "fbr_mesh_bvh_grad.h", "fbr_mesh_bvh.h", "fbr_mesh_grad.h", "fbr_mesh.h", "fbr_hull_grad.h", "fbr_hull.h", "fbr_box_grad.h", "fbr_box.h",
            "fbr_capsule_grad.h", "fbr_capsule.h", "fbr_math.h", "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
        _lib.meshbvhgrad_entry.restype = ctypes.c_long
    return _lib


def model_arrays(topo):
    return (_c(topo.parent, np.int32), _c(topo.dof_index, np.int32), _c(topo.rest_R).reshape(-1), _c(topo.rest_p).reshape(-1), _c(topo.axis).reshape(-1),
            _c(topo.joint_type, np.int32))


def hull_arrays(topo, hulls):
    link = _c(link_index(topo, hulls), np.int32)
    off = _c([h.offset for h in hulls]).reshape(-1)
    rot = _c([np.eye(3) if h.rot is None else h.rot for h in hulls]).reshape(-1)
    return (link, off, rot) + tuple(tables(hulls)[:6])


SMAX = 2 * 7 + 1  # the stencil points of a pair at most, on the robots of these tests


def tree_items(topo, hulls, meshes, item_pairs, q, mode, eps, route, C=None):
    """(dist (M,), grad (M, n), stencil points (M,), stats) of one hull pair per configuration, fixed base.  Routes 0 and 1: any M items;
    2 and 3: M = C K items, item c K + k the pair k of candidate c, the packets of a pair formed over its C candidates; stats["stencil"]
    (M, SMAX) then holds the stencil values of every item, NaN behind its last."""
    parent, dof, rR, rp, ax, jt = model_arrays(topo)
    link, off, rot, vbeg, v, fbeg, pl, ebeg, ed = hull_arrays(topo, hulls)
    mtab, tris = tm.mesh_tables(len(hulls), meshes)
    pr = _c(item_pairs, np.int32).reshape(-1, 2)
    q = _c(q)
    M = q.shape[0]
    assert len(pr) == M
    C = M if C is None else int(C)
    K = M // C
    assert C * K == M
    dist, grad, ns, stats = np.zeros(M), np.full((M, topo.num_dofs), np.nan), np.zeros(M, dtype=np.int32), np.zeros(6, dtype=np.int64)
    stencil = np.full((M, SMAX), np.nan)
    rc = emul().meshbvhgrad_eval(topo.num_links, topo.num_dofs, _p(parent), _p(dof), _p(rR), _p(rp), _p(ax), _p(jt), 0, len(hulls), _p(link), _p(off),
                                 _p(rot), int(mode), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), _p(mtab), _p(tris), ctypes.c_long(len(tris)),
                                 ctypes.c_double(eps), ctypes.c_long(C), ctypes.c_long(K), _p(pr), _p(q), None, None, int(route), _p(dist), _p(grad),
                                 _p(ns), stats.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), SMAX, _p(stencil))
    assert rc == 0, rc
    return dist, grad, ns, dict(zip(STATS, (int(x) for x in stats)), stencil=stencil)


def tree_evaluate(case, C, sample, scale, pose, eps, mode, route=1, pairs=None):
    """the contract of fbr_large_mesh_distance_gradients for the MESH pairs of a fixed-base case {topo, hulls, meshes, pairs, q (C T, n)} from
    the emulation: (dist (C, P), grad (C, P, n), stencil points (C, P), stats)"""
    pairs = np.asarray(case["pairs"] if pairs is None else pairs).reshape(-1, 2)
    P, Tn = len(pairs), case["q"].shape[0] // C
    sample = np.asarray(sample).reshape(C, P)
    sc = np.ones((C, P)) if scale is None else np.asarray(scale)
    rq = ((np.arange(C) * Tn)[:, None] + np.maximum(sample, 0)).reshape(-1)
    dist, grad, ns, stats = tree_items(case["topo"], case["hulls"], case["meshes"], np.tile(pairs, (C, 1)), case["q"][rq] * sc.reshape(-1, 1), mode, eps,
                                       route, C=C)
    none = sample < 0
    return np.where(none, NONE, dist.reshape(C, P)), np.where(none[..., None], 0.0, grad.reshape(C, P, -1)), ns.reshape(C, P), stats


# ---- (a) the stages equal the single pass ---------------------------------------------------------------------------------------------------------
KINDS = ("soupL", "soupL1", "soup2L1", "soup257", "blob x blob", "sphere on 132 vertices x box", "sphere on 132 vertices x 129 vertices", "torus")
POSTURE = np.array([0.3, 1.2, -0.4, -1.5, 0.5, 0.9, 0.2])
NC = 3  # candidates a case


def chain_case(kind, mode):
    """hulls 0 (a mesh, lwr_2_link), 1 (lwr_5_link: a mesh or a solid), 2 (a world box on a vertex of mesh 0 at the first configuration), 3 (a
    world box a metre away); K = 6 pairs a candidate: (0, 1), (1, 0), (0, 2), (2, 0), (0, 3), (1, 3) -- (1, 3) only where 1 has a mesh --;
    q (NC K, 7): the first configuration shared by the items of candidate 0, a NaN in joint 4 of item (1, 0)"""
    from flobaroid_amd.collision import Hull

    topo = load_topo("kuka_lwr4")
    s = tl.shapes()
    rng = np.random.default_rng(KINDS.index(kind) + 50)
    box = lambda half: hs.box([half] * 3)  # noqa: E731
    if kind.startswith("soup"):
        A, B = ml.hull_of(s[kind], "lwr_2_link", offset=[0.0, -0.25, 0.0]), ml.hull_of(s["soup2L1"] if kind != "soup2L1" else s["soupL1"], "lwr_5_link",
                                                                                     offset=[0.0, 0.2, 0.0])
        meshes = {0: s[kind], 1: s["soup2L1"] if kind != "soup2L1" else s["soupL1"]}
    elif kind == "blob x blob":
        A, B = ml.hull_of(s["blob"], "lwr_2_link", offset=[0.0, -0.25, 0.0]), ml.hull_of(s["blob2"], "lwr_5_link", offset=[0.0, 0.2, 0.0])
        meshes = {0: s["blob"], 1: s["blob2"]}
    elif kind.startswith("sphere"):
        A = ml.hull_of(s["sphere"], "lwr_2_link", pad=None, offset=[0.0, -0.25, 0.0])
        B = Hull("lwr_5_link", box(0.08), np.array([0.0, 0.2, 0.0])) if kind.endswith("box") else hl.on(hl.shape("sphere129"), "lwr_5_link", [0.0, 0.2, 0.0])
        meshes = {0: s["sphere"]}
        assert len(A.vertices) == 132 and len(B.vertices) == (8 if kind.endswith("box") else 129)
    else:
        A, B = ml.hull_of(s["torus"], "lwr_2_link", offset=[0.0, -0.25, 0.0]), ml.hull_of(s["soup2L1"], "lwr_5_link", offset=[0.0, 0.2, 0.0])
        meshes = {0: s["torus"], 1: s["soup2L1"]}
    K = 6 if 1 in meshes else 5
    q = POSTURE + rng.uniform(-0.3, 0.3, (NC, 1, 7)) + rng.uniform(-0.02, 0.02, (NC, K, 7))
    q[0, :] = q[0, 0]
    R, cen = hr.hull_world(topo, as_tuples(topo, [A]), q[0, :1], False, None, None, mode)
    touch = cen[0, 0] + R[0, 0] @ meshes[0][0, 0]
    hulls = [A, B, Hull(None, box(0.05), touch, rot=np.eye(3), name="touch"), Hull(None, box(0.05), touch + np.array([0.6, 0.8, 0.3]), rot=np.eye(3), name="far")]
    pairs = np.array([(0, 1), (1, 0), (0, 2), (2, 0), (0, 3), (1, 3)][:K], dtype=np.int32)
    q[1, 0, 3] = np.nan
    return {"topo": topo, "hulls": hulls, "meshes": meshes, "pairs": pairs, "q": np.ascontiguousarray(q.reshape(NC * K, 7)), "K": K}


# every shape in world axes, the mode with more stencil points; four of them in link axes as well
CASES = [(k, False) for k in KINDS] + [(k, True) for k in ("soup2L1", "soup257", "sphere on 132 vertices x box", "sphere on 132 vertices x 129 vertices")]


@pytest.mark.parametrize("kind,mode", CASES, ids=[f"{k}-{'link' if m else 'world'}-axes" for k, m in CASES])
def test_tree_stages_equal_the_brute_force_single_pass_bit_for_bit(kind, mode):
    case = chain_case(kind, mode)
    K, topo = case["K"], case["topo"]
    item_pairs = np.tile(case["pairs"], (NC, 1))
    d0, g0, n0, _ = tree_items(topo, case["hulls"], case["meshes"], item_pairs, case["q"], mode, 1e-7, 0)
    d1, g1, n1, s1 = tree_items(topo, case["hulls"], case["meshes"], item_pairs, case["q"], mode, 1e-7, 1)
    nan = np.isnan(d0)
    same = lambda a, b: np.array_equal(np.isnan(a), np.isnan(b)) and a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()  # noqa: E731
    assert same(d0, d1) and same(g0, g1)
    # the NaN pose: one item, NaN in the distance and in the evaluated entries only
    assert nan.sum() == 1 and nan[K] and not np.isnan(g1[~nan]).any()
    on_nan = np.isnan(g1[K])
    assert on_nan.sum() == (n1[K] - 1) // 2 and np.all(g1[K][~on_nan] == 0.0)
    # the touching centre: both orders of (mesh 0, the world box on its vertex) at the first configuration
    for k in (2, 3):
        assert d1[k] == 0.0 and not g1[k].any() and n1[k] >= 5
    # the stencil: the centre and two points a joint; a world member leaves the joints above the robot link, a pair on the chain those
    # between its links (and, in world axes, the revolute joints above both)
    assert np.all(n1 % 2 == 1) and np.all(n1[[0, 1]] == (11 if not mode else 7)) and np.all(n1[[2, 3, 4]] == 5)
    touched = np.array([(g1[i] != 0.0) | np.isnan(g1[i]) for i in range(len(g1))])
    assert not touched[:, 5:].any() and not touched[2:5, 2:].any() and touched.any(axis=0)[:5].all()
    if mode:
        assert not touched[:2, :2].any()
    apart = ~nan & (d1 > 0)
    assert apart.sum() >= NC * 2 and np.abs(g1[apart]).max() > 1e-2
    # the stages as the waves run them, in both orders
    for route in (2, 3):
        dp, gp, npk, sp = tree_items(topo, case["hulls"], case["meshes"], item_pairs, case["q"], mode, 1e-7, route, C=NC)
        assert same(dp, d1) and same(gp, g1) and np.array_equal(npk, n1)
        assert sp["walks"] == sum(-(-int(n1[k]) * NC // 64) for k in range(K))
    nt = [len(case["meshes"][h]) if h in case["meshes"] else 1 for h in range(4)]
    brute = int(sum(int(n1[i]) * nt[a] * nt[b] for i, (a, b) in enumerate(item_pairs)))
    print(f"{kind} mode {int(mode)}: {len(d1)} items, {int(n1.sum())} stencil entries; the walks evaluated {s1['evals']} of {brute} triangle pairs "
          f"({s1['evals'] / brute:.3%}), {s1['node_pairs']} node pairs, stack {s1['max_stack']}; distances {np.nanmin(d1):.4f} .. {np.nanmax(d1):.4f}")


# ---- (b) the entry mapping ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [CANDIDATE_MAJOR, SLOT_MAJOR], ids=["candidate-major", "slot-major"])
def test_entry_mapping_is_a_bijection(order):
    for S in (1, 3, 63, 64, 65):
        for C in (1, 65):
            seen = np.zeros((S, C), dtype=int)
            s, c = ctypes.c_int32(0), ctypes.c_int64(0)
            for e in range(S * C):
                back = emul().meshbvhgrad_entry(order, ctypes.c_long(e), S, ctypes.c_long(C), ctypes.byref(s), ctypes.byref(c))
                assert back == e and 0 <= s.value < S and 0 <= c.value < C
                assert (s.value, c.value) == ((e % S, e // S) if order == CANDIDATE_MAJOR else (e // C, e % C))
                seen[s.value, c.value] += 1
            assert np.all(seen == 1)
            # the tiles as the kernel cuts them (fbr_mesh_bvh_grad_tile): no lane's entry leaves the pair, every entry is stored once
            E, e0 = S * C, ctypes.c_int64(0)
            stored = np.zeros(E, dtype=int)
            for t in range(-(-E // 64) + 1):
                valid = emul().meshbvhgrad_tile(ctypes.c_long(t), ctypes.c_long(E), ctypes.byref(e0))
                assert (valid == 0) == (t == -(-E // 64)) and 0 <= valid <= 64
                if valid:
                    lanes = e0.value + np.minimum(np.arange(64), valid - 1)
                    assert lanes.min() >= 0 and lanes.max() < E
                    stored[lanes[:valid]] += 1
            assert np.all(stored == 1)
    assert emul().meshbvhgrad_default_order() in (CANDIDATE_MAJOR, SLOT_MAJOR)


# ---- (c) under the sanitizers -----------------------------------------------------------------------------------------------------------------------
def test_tables_mapping_and_restatement_under_the_sanitizers(tmp_path):
    """tests/emul/mesh_bvh_grad_sanitize.cpp, a program of its own, built with -fsanitize=address,undefined and run here on the CPU on the
    smallest shapes: soupL on lwr_2_link, soupL1 on lwr_5_link, the sphere on its 132 vertices (a BIG pair against the far box), two boxes"""
    exe = str(tmp_path / "mesh_bvh_grad_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(_HERE, "emul", "mesh_bvh_grad_sanitize.cpp")])
    case = chain_case("soupL", False)
    s = tl.shapes()
    topo = case["topo"]
    hulls = case["hulls"] + [ml.hull_of(s["sphere"], "lwr_4_link", pad=None)]
    case["hulls"][1] = hulls[1] = ml.hull_of(s["soupL1"], "lwr_5_link", offset=[0.0, 0.2, 0.0])
    meshes = {0: s["soupL"], 1: s["soupL1"]}
    set_pairs = np.array([(0, 1), (4, 3), (1, 0), (0, 2), (4, 1), (2, 4), (1, 3)], dtype=np.int32)  # MESH, BIG, MESH, MESH, MESH, BIG, MESH
    parent, dof, rR, rp, ax, jt = model_arrays(topo)
    link, off, rot, vbeg, v, fbeg, pl, ebeg, ed = hull_arrays(topo, hulls)
    mtab, tris = tm.mesh_tables(len(hulls), meshes)
    K = case["K"]
    q = np.where(np.isnan(case["q"]), 0.25, case["q"])
    words = []
    for a in (topo.num_links, topo.num_dofs, parent, dof, jt, rR, rp, ax, len(hulls), link, off, rot, vbeg, v, fbeg, pl, ebeg, ed, mtab, len(tris), tris,
              len(set_pairs), set_pairs, NC, K, np.tile(case["pairs"], (NC, 1)), q):
        words += [repr(x) for x in np.asarray(a).reshape(-1).tolist()]
    run = subprocess.run([exe], input=" ".join(words), capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and not run.stderr, (run.stdout, run.stderr[-2000:])
    assert int(run.stdout.split()[2]) == NC * K


# ---- (d) excitation: the keyword against a stub engine ------------------------------------------------------------------------------------------------
class _Hull:
    def __init__(self, name, nv):
        self.link_name, self.name, self.vertices = name, name, np.zeros((nv, 3))


class StubEngine:
    """tests/test_meshes_large.py RecordingEngine with the gradient calls: marks what the new call returns, rows 9000 + 10 pair + joint; the
    chain is the identity padded to the chain's width"""
    floating, n = False, 3

    def __init__(self):
        self.calls = []

    def set_capsules(self, *a, **k):
        raise AssertionError("a hull set installs no capsules")

    set_boxes = set_capsules

    def set_hulls(self, hulls, pairs, offset_in_link_axes=False, **kw):
        self.P = len(pairs)
        self.calls.append(("set_hulls", offset_in_link_axes, {k: (v if isinstance(v, bool) else sorted(v)) for k, v in kw.items()}))

    def candidate_hull_distances(self, st, ncand, step=3, base_pos=None, device_out=None):
        return {"dist": np.full((ncand, self.P), 0.5), "idx": np.zeros((ncand, self.P), dtype=np.int64)}

    def hull_distance_gradients(self, *a, **k):
        raise AssertionError("a set with large_meshes goes to large_mesh_distance_gradients")

    mesh_distance_gradients = large_hull_distance_gradients = hull_distance_gradients

    def large_mesh_distance_gradients(self, st, C, sample, scale=None, pose_sample=None, base_pos=None, epsilon=None):
        self.calls.append(("large_mesh_gradients", epsilon))
        P = self.P
        assert sample.shape == scale.shape == pose_sample.shape == (C, P)
        assert np.array_equal(sample, np.tile(np.arange(P) + 300, (C, 1))) and np.array_equal(pose_sample, sample + 1) and np.array_equal(scale, sample * 0.5)
        return {"dist": np.zeros((C, P)), "grad_q": 9000.0 + 10.0 * np.arange(P)[None, :, None] + np.arange(self.n)[None, None, :] + np.zeros((C, 1, 1))}

    def fourier_position_chain(self, wf, A, B, sample, grad_q, freq, scale=None, q_range=None):
        C, P, n = grad_q.shape
        out = np.zeros((C, P, 1 + 2 * n + 2 * n * A.shape[2]))
        out[:, :, 1:1 + n] = grad_q
        return out


def test_large_mesh_rows_against_a_stub_engine():
    from flobaroid_amd import excitation as exc

    C, n, nh = 2, 3, 2
    columns = np.array([[2, 2], [2, 0], [2, 3], [2, 1]])  # the reference's order: hull pairs 2, 0, 3, 1
    big = [_Hull("base", 216), _Hull("lwr_6_link", 793), _Hull("lwr_7_link", 158), _Hull("tool", 12)]
    tri = lambda k: np.zeros((k, 3, 3))  # noqa: E731
    cs = {"capsules": [], "pairs": np.zeros((0, 2)), "hulls": big, "hull_pairs": np.array([(0, 1), (0, 2), (1, 3), (2, 3)]), "columns": columns,
          "offset_in_link_axes": True, "meshes": {0: tri(4434), 2: tri(1098)}, "large_meshes": True}
    small = dict(cs, hulls=[_Hull(h.name, min(len(h.vertices), 128)) for h in big])
    P = len(columns)
    own = columns[:, 1] + 300
    cons = {"g": np.arange(C * P, dtype=float).reshape(C, P), "eval_sample": np.tile(own, (C, 1)), "eval_scale": np.tile(own, (C, 1)) * 0.5,
            "eval_pose": np.tile(own, (C, 1)) + 1}
    cand = [{"wf": 1.0, "a": np.zeros((n, nh)), "b": np.zeros((n, nh)), "q_range": None}] * C
    st = {"q": np.zeros((C * 4, n))}
    full = {"collisionMode": "full", "analyticalGradientEpsilon": 3e-6}
    links = {"collisionMode": "convex", "fullMeshLinks": ["base"], "analyticalGradientEpsilon": 3e-6}
    want = 9000.0 + 10.0 * columns[:, 1][None, :, None] + np.arange(n)[None, None, :] + np.zeros((C, 1, 1))
    # the keyword routes the set -- large_meshes, and large where a hull exceeds 128 vertices -- to the new call, whatever the others say
    for config in (full, links):
        for cset, large in ((cs, True), (small, False)):
            for kw, eps in (({}, 3e-6), ({"mesh_gradient": True, "hull_gradient": True}, 3e-6), ({"large_hull_gradient": True, "epsilon": 1e-5}, 1e-5)):
                eng = StubEngine()
                out = exc.candidate_collision_gradient(eng, st, C, cand, 50.0, config, cset, constraints=cons, large_mesh_gradient=True, **kw)
                assert np.array_equal(out["grad_q"], want) and np.array_equal(out["grad"]["q_offset"], want) and np.array_equal(out["g"], cons["g"])
                assert out["grad"]["a"].shape == (C, P, n, nh) and not out["grad"]["a"].any() and not out["grad"]["wf"].any()
                kws = dict({"large": True} if large else {}, meshes=[0, 2], large_meshes=True)
                assert eng.calls == [("set_hulls", True, kws), ("large_mesh_gradients", eps)]
    # without the keyword: the refusal of before, word for word, whatever the other keywords say
    text = ("gradients on the device do not cover triangle meshes of more than 256 triangles or on hulls of more than 128 vertices: the collision set was "
            "built with large_meshes=True and has base (4434 triangles on a hull of 216 vertices), lwr_7_link (1098 triangles on a hull of 158 vertices); the "
            "constraint values are served (Engine.set_large_hull_meshes), their gradients are not built")
    for kw in ({}, {"hull_gradient": True}, {"mesh_gradient": True}, {"large_hull_gradient": True}, {"box_gradient": True}, {"large_mesh_gradient": False}):
        with pytest.raises(ValueError) as e:
            exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, full, cs, constraints=cons, **kw)
        assert str(e.value) == text
        with pytest.raises(ValueError) as e:
            exc.candidate_gradients_from_coefficients(StubEngine(), cand, 4, 50.0, None, None, {}, [], full, collision=cs, **kw)
        assert str(e.value) == text
    # every new ValueError says which condition fails and, where one exists, names the keyword that serves the set
    no_flag = {k: v for k, v in small.items() if k != "large_meshes"}
    no_mesh_big = {k: v for k, v in cs.items() if k not in ("large_meshes", "meshes")}
    no_mesh_small = {k: v for k, v in small.items() if k not in ("large_meshes", "meshes")}
    mixed = dict(cs, columns=np.array([[2, 0], [1, 0], [2, 1], [2, 2]]))
    for config, cset, msg in (({"collisionMode": "capsule"}, cs, "collisionMode 'capsule' has no triangle meshes"),
                              ({"collisionMode": "box"}, cs, "collisionMode 'box' has no triangle meshes"),
                              (full, no_flag, r"not built with large_meshes=True .*; mesh_gradient=True serves"),
                              (full, no_mesh_big, r"not built with large_meshes=True .*; large_hull_gradient=True serves"),
                              (full, no_mesh_small, r"not built with large_meshes=True .*; hull_gradient=True serves"),
                              ({"collisionMode": "convex"}, cs, "collisionMode 'convex' without fullMeshLinks"),
                              (full, mixed, "capsule or box pairs"),
                              (full, {"capsules": ["c"] * 2, "pairs": [(0, 1)], "hulls": big, "meshes": cs["meshes"], "large_meshes": True}, "needs hull pairs")):
        with pytest.raises(ValueError, match="large_mesh_gradient=True: .*" + msg):
            exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, config, cset, constraints=cons, large_mesh_gradient=True)
        with pytest.raises(ValueError, match="large_mesh_gradient=True: .*" + msg):
            exc.candidate_gradients_from_coefficients(StubEngine(), cand, 4, 50.0, None, None, {}, [], config, collision=cset, large_mesh_gradient=True)
    with pytest.raises(ValueError, match=r"large_mesh_gradient=True: no collision set"):
        exc.candidate_gradients_from_coefficients(StubEngine(), cand, 4, 50.0, None, None, {}, [], full, large_mesh_gradient=True)
    # the suspended base stays refused in the gradient path
    with pytest.raises(ValueError, match="suspended"):
        exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, dict(full, floatingBaseAttachment="suspended"), cs, constraints=cons,
                                         large_mesh_gradient=True)
    for f in (exc.candidate_collision_gradient, exc.candidate_collision_gradient_from_coefficients, exc.candidate_gradients_from_coefficients):
        assert inspect.signature(f).parameters["large_mesh_gradient"].default is False
    # the constraint block of such a set is installed the same way (tests/test_meshes_large.py RecordingEngine)
    eng = StubEngine()
    exc._collision_block(eng, {"q": st["q"], "dq": st["q"], "ddq": st["q"]}, C, dict(full, collisionCheckStep=1, transitionDuration=0.0), cs)
    assert eng.calls == [("set_hulls", True, {"meshes": [0, 2], "large": True, "large_meshes": True})]


# ---- (e) the symbol -------------------------------------------------------------------------------------------------------------------------------------
def test_large_mesh_gradient_symbol_in_header_binding_and_library():
    """added under C-ABI 104: the version stays; header, binding and library carry the symbol and the option"""
    from flobaroid_amd import _lib

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    name = "fbr_large_mesh_distance_gradients"
    assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr)
    assert _lib._SIGNATURES[name] == _lib._SIGNATURES["fbr_mesh_distance_gradients"]
    assert lib.fbr_version() == _lib.FBR_VERSION == 104 == int(re.search(r"#define FBR_VERSION (\d+)", hdr).group(1))
    assert hasattr(_lib.Engine, "large_mesh_distance_gradients")
    assert list(inspect.signature(_lib.Engine.large_mesh_distance_gradients).parameters) == list(inspect.signature(_lib.Engine.mesh_distance_gradients).parameters)
    assert "distances only" not in _lib.Engine.set_large_hull_meshes.__doc__.lower()
    opts = open(os.path.join(_CSRC, "fbr_options.h")).read()
    assert '"mesh_grad_order"' in hdr and '"mesh_grad_order"' in opts and "hull_large_all" in hdr.split("int " + name)[0].rsplit("/*", 1)[1]
    names, i, p = [], 0, ctypes.c_char_p()
    while lib.fbr_model_option_name(i, ctypes.byref(p)) == 0:
        names.append(p.value.decode())
        i += 1
    assert "mesh_grad_order" in names
    api = open(os.path.join(_CSRC, "fbr_collision_api.hip")).read()
    assert "fbr_mesh_bvh_grad.h" in api and "fbr_mesh_bvh_grad_dist_kernel" in api
    assert lib.fbr_large_mesh_distance_gradients(None, None, None, 1, None, None, None, 1e-7, None, None, 0) == -1  # FBR_E_INVALID: no model
