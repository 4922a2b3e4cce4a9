"""fbr_model_set_large_hull_meshes / fbr_candidate_hull_distances with meshes behind a tree on the device (csrc/fbr_mesh_bvh.h) against the
g++ emulation of the same text walked over packets of 64 poses (tests/emul/mesh_bvh_emul.cpp, on the frames of tests/emul/hull_emul.cpp)
and the restatement of tests/mesh_restatement.py.

(a) the left arm under the crane of tests/test_gpu_meshes.py, its small meshes installed once by each entry point: identical bytes, both
kernels on the same frames.  (b) the shapes of tests/mesh_large_shapes.py on the gantry of tests/hull_shapes.py, its carriage turned by
pi / 4: torus x sheet, (c) blob x blob (182 x 182 triangle pairs), a soup of 257 against the sphere on its hull of 132 vertices, meshes
against a box, a prism and a plain hull of 129 vertices, beside plain pairs of small and of large hulls; C = 2 and 1, 63 and 65 checked
samples a candidate, host and device states.  Indices equal the emulation's; values within the bar of tests/test_gpu_meshes.py: the
larger of 10 x the deviation of the emulation from the restatement measured on the same inputs (the winning samples) and 32 eps x the
pair's scale -- for 1 and 63 samples, where the restatement is not run, 32 eps x scale alone.  (d) one block a launch, each candidate
alone, pairs and meshes shuffled, two runs: the same bits.  (e) pairs without a mesh: the bytes of the set without meshes.  (f) refused
calls leave the attachments in place.  (g) KUKA LWR4, collisionMode "full", from the STL files of tests/golden/urdf/meshes/kuka and
world_kuka.urdf through candidate_objectives_from_coefficients.

Seen on an MI355X: (a) identical bytes; (b), (c) the emulation's bits on every pair at 1, 63 and 65 samples (|device - emulation| = 0;
emulation - restatement 1.1e-16, smallest bar 1.3e-14; the tree evaluated 1.5 % of the 5.6e7 triangle pairs of the 65-sample case); (g) 29
pairs, every value within the bar of the emulation at the winning configuration ("Large triangle meshes behind a tree").
The references take half a minute on the CPU, once a session, most of it the restatement at the 18 winning samples."""
import functools
import os

import numpy as np
import pytest

import hull_large_shapes as hl
import hull_restatement as hr
import hull_shapes as hs
import mesh_large_shapes as ml
import mesh_restatement as mr
import test_meshes_large as tl
from common import GOLDEN, load_topo, random_states
from test_gpu_boxes import _engine, _host
from test_gpu_meshes import call, is_mesh_pair, same
from test_hulls import EPS, as_tuples, emul_eval, left_arm_hulls

pytestmark = pytest.mark.gpu
URDF = os.path.join(GOLDEN, "urdf")


def frames_of(topo, hulls, q, mode=False):
    """(S, H, 12): the frames of the library's own lane walk on the CPU (tests/emul/hull_emul.cpp), through four-vertex stand-ins on the same
    links -- a frame does not depend on the vertices, and that emulation takes small hulls only"""
    from flobaroid_amd.collision import Hull

    tetra = Hull("t", np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), np.zeros(3))
    stand = [hl.on(tetra, h.link_name, h.offset, h.rot, h.name) for h in hulls]
    return emul_eval(topo, False, stand, np.zeros((0, 2), dtype=np.int32), q, None, None, mode)[0]


# ---- (a) small meshes through either entry point -----------------------------------------------------------------------------------------------
def test_small_meshes_give_the_same_bytes_through_either_entry_point():
    """the construction of tests/test_gpu_meshes.py's left_arm_case (without its references): C = 3, T = 200, step 3"""
    import test_meshes as tm
    from flobaroid_amd.collision import Box, hull_from_box, world_hulls_from_urdf

    C, T, STEP = 3, 200, 3
    rng = np.random.default_rng(12)
    topo, (hulls, _) = left_arm_hulls()
    ms = tm.fixture_meshes()
    b = hulls["LShr"].bounds
    hulls["LShr"] = hull_from_box(Box("LShr", 0.5 * (b[1] - b[0]), hulls["LShr"].offset + 0.5 * (b[0] + b[1])))
    wh = world_hulls_from_urdf(os.path.join(URDF, "world_walkman_suspended.urdf"), "geometric")
    hlist = [hulls[n] for n in topo.link_names if n in hulls] + list(wh.values())
    at = {(h.link_name or h.name): i for i, h in enumerate(hlist)}
    meshes = {at["LSoftHandLink"]: ms["LSoftHandLink"].triangles, at["LForearm"]: ms["LForearm"].triangles}
    st = random_states(topo, C * T, rng, True, use_limits=True)
    st["rpy"] = rng.uniform(-0.6, 0.6, (C * T, 3))
    bp = wh["crane_tip"].offset + rng.standard_normal((C * T, 3)) * 0.15
    want = [("LForearm", "LSoftHandLink"), ("LShp", "LForearm"), ("LShr", "LForearm"), ("LSoftHandLink", "crane_arm"),
            ("Waist", "LElb"), ("LShp", "LElb"), ("LShr", "LWrMot2"), ("LShy", "crane_tip"), ("LElb", "crane_arm")]
    pairs = np.array(sorted((at[a], at[b]) for a, b in want), dtype=np.int32)
    eng = _engine(topo, True)
    eng.set_hulls(hlist, pairs, offset_in_link_axes=True, meshes=meshes)
    old = call(eng, st, bp, C, STEP, True)
    eng.set_hulls(hlist, pairs, offset_in_link_axes=True, meshes=meshes, large_meshes=True)
    new = call(eng, st, bp, C, STEP, True)
    assert same(old, new)
    eng.set_hull_meshes(meshes)  # back, in place
    assert same(call(eng, st, bp, C, STEP, False), old)
    eng.set_large_hull_meshes(meshes)
    assert same(call(eng, st, bp, C, STEP, False), old)
    mp = is_mesh_pair(pairs, meshes)
    assert np.isfinite(old["dist"]).all() and (old["dist"][:, mp] >= 0).all() and mp.sum() == 4


# ---- (b), (c) the large shapes on the gantry ------------------------------------------------------------------------------------------------------
C = 2


@functools.lru_cache(maxsize=None)
def gantry_set():
    """hulls, meshes {hull: triangles}, pairs: three robot links, the carriage turned by pi / 4 about x; offsets in world axes"""
    from flobaroid_amd.collision import Hull

    topo = hs.turned_gantry("quarter")
    s = tl.shapes()
    soup = ml.soup(4, 257, 0.05)
    hulls = [ml.hull_of(s["torus"], "bed", offset=[0.25, 0.0, 0.0]),                       # 0 mesh
             ml.hull_of(s["sheet"], "carriage", offset=[0.0, 0.0, -0.35]),                  # 1 mesh
             ml.hull_of(s["blob"], "bed", offset=[1.5, 0.0, 0.0]),                          # 2 mesh
             ml.hull_of(s["blob2"], "carriage", offset=[1.25, 0.0, -0.05]),                 # 3 mesh
             ml.hull_of(s["sphere"], "carriage", pad=None, offset=[-1.75, 0.0, -0.05]),     # 4 mesh on a hull of 132 vertices
             ml.hull_of(soup, "bed", offset=[-1.5, 0.0, -0.1]),                             # 5 mesh
             Hull("column", hs.box([0.0625, 0.0625, 0.0625]), np.array([0.0, 1.5, 0.0])),   # 6 a box
             Hull("bed", hs.prism(64, 0.25, 0.5), np.array([0.25, 0.6, 0.0])),              # 7 a prism of 128 vertices
             hl.on(hl.shape("sphere129"), "bed", [-1.5, 1.5, 0.0])]                         # 8 a plain hull of 129 vertices
    meshes = {0: s["torus"], 1: s["sheet"], 2: s["blob"], 3: s["blob2"], 4: s["sphere"], 5: soup}
    # torus x sheet, blob x blob, soup x sphere-on-large-hull, mesh x box, mesh x prism, mesh-on-large-hull x prism, mesh x large plain
    # hull; plain: box x prism (small), box x sphere129 (large)
    pairs = np.array([(0, 1), (2, 3), (5, 4), (0, 6), (1, 7), (4, 7), (8, 3), (6, 7), (6, 8)], dtype=np.int32)
    return topo, hulls, meshes, pairs


def gantry_states(T, seed):
    rng = np.random.default_rng(seed)
    # a smooth path a candidate, as a trajectory's samples: lift within [0.05, 0.3], slide within [-0.2, 0.2]
    t = np.linspace(0.0, 1.0, T)[None, :] if T > 1 else np.zeros((1, 1))
    ph = rng.uniform(0, 2 * np.pi, (C, 2, 1))
    lift = 0.175 + 0.125 * np.sin(2 * np.pi * 1.3 * t + ph[:, 0])
    slide = 0.2 * np.sin(2 * np.pi * 0.7 * t + ph[:, 1])
    return {"q": np.ascontiguousarray(np.stack([lift, slide], axis=2).reshape(C * T, 2))}


@functools.lru_cache(maxsize=None)
def gantry_reference(T, restate):
    """(states, emulation's minima (C, P), indices, bar (C, P), brute-force statistics) -- asserted on the way: the tree's bits are the
    brute force's on every sample; with ``restate`` the restatement at the winning samples is clear of the grey zone and within the bar"""
    topo, hulls, meshes, pairs = gantry_set()
    st = gantry_states(T, 40 + T)
    fr = frames_of(topo, hulls, st["q"])
    emu, sa, sb = tl.same_bits(fr, hulls, meshes, pairs, ("gantry", T))
    val, idx = hr.candidate_minimum(emu, C, 1)
    tup = as_tuples(topo, hulls)
    R, cen = hr.hull_world(topo, tup, st["q"], False, None, None, False)
    diam = np.array([h.diameter for h in hulls])
    bar, dev = np.zeros((C, len(pairs))), 0.0
    mp = is_mesh_pair(pairs, meshes)
    for c in range(C):
        for k, (a, b) in enumerate(pairs):
            s = c * T + int(idx[c, k])
            bar[c, k] = 32.0 * EPS * (np.linalg.norm(cen[s, b] - cen[s, a]) + diam[a] + diam[b])
    if restate:
        want = np.zeros((C, len(pairs)))
        for c in range(C):
            for k, (a, b) in enumerate(pairs):
                s = c * T + int(idx[c, k])
                if mp[k]:
                    sg = mr.mesh_signed(R[s, a], cen[s, a], meshes.get(int(a)), hulls[a].vertices, R[s, b], cen[s, b], meshes.get(int(b)), hulls[b].vertices)
                    assert abs(sg) > 100.0 * bar[c, k], ("grey zone: change the seed", c, k, sg)
                    want[c, k] = float(mr.clamp(sg))
                else:
                    want[c, k] = hr.hull_distance(R[s, a], cen[s, a], hulls[a].vertices, R[s, b], cen[s, b], hulls[b].vertices)
        dev = float(np.abs(val - want).max())
        bar = np.maximum(bar, 10.0 * dev)
        assert np.all(np.abs(val - want) <= bar)
    print(f"gantry reference, T = {T}: emulation - restatement {dev:.3e}, smallest bar {bar.min():.3e}; the tree evaluated {sa['evals']} of "
          f"{sb['all_pairs']} triangle pairs ({sa['evals'] / max(sb['all_pairs'], 1):.3%}), {sa['node_pairs']} node pairs, stack {sa['max_stack']}; minima {val.min():.4f} .. {val.max():.4f}")
    assert np.all(val[:, mp] > 0.0), "the gantry's mesh pairs stay apart"
    return st, val, idx, bar


def install(eng, large_meshes=True, pairs=None, meshes=None):
    topo, hulls, m, p = gantry_set()
    eng.set_hulls(hulls, p if pairs is None else pairs, large=True, meshes=m if meshes is None else meshes, large_meshes=large_meshes)


@pytest.mark.parametrize("T", [65, 63, 1])
def test_large_shapes_on_the_gantry(T):
    topo, hulls, meshes, pairs = gantry_set()
    st, val, idx, bar = gantry_reference(T, T == 65)
    eng = _engine(topo, False)
    install(eng)
    a = call(eng, st, None, C, 1, False)
    b = call(eng, st, None, C, 1, True)
    err = np.abs(a["dist"] - val)
    print(f"gantry T = {T}: max |device - emulation| = {err.max():.3e} = {(err / bar).max():.3f} bars ({'the same bits' if err.max() == 0 else 'not the same bits'})")
    assert same(a, b)
    assert np.array_equal(a["idx"], idx)
    assert np.all(err <= bar)
    # (e) the pairs without a mesh return the bytes of the same set without meshes
    mp = is_mesh_pair(pairs, meshes)
    eng.set_hulls(hulls, pairs, large=True)
    plain = call(eng, st, None, C, 1, True)
    assert a["dist"][:, ~mp].tobytes() == plain["dist"][:, ~mp].tobytes() and np.array_equal(a["idx"][:, ~mp], plain["idx"][:, ~mp])
    assert np.all(a["dist"][:, mp] >= plain["dist"][:, mp] - bar[:, mp])  # a mesh is never nearer than its hull
    eng.close()


def test_variants_give_the_same_bits():
    """(d): two runs, one block a launch, each candidate alone, the pair list shuffled (the same columns), the mesh list shuffled; (e) with
    every pair through the large-hull kernel (option hull_large_all)"""
    T = 65
    topo, hulls, meshes, pairs = gantry_set()
    st, val, idx, bar = gantry_reference(T, True)
    eng = _engine(topo, False)
    install(eng)
    a = call(eng, st, None, C, 1, True)
    assert same(call(eng, st, None, C, 1, True), a)
    eng2 = _engine(topo, False, options={"chunk_samples": 64})
    install(eng2)
    assert same(call(eng2, st, None, C, 1, True), a)
    for k in range(C):
        one = call(eng, st, None, 1, 1, True, slice(k * T, (k + 1) * T))
        assert one["dist"].tobytes() == a["dist"][k:k + 1].tobytes() and one["idx"].tobytes() == a["idx"][k:k + 1].tobytes()
    perm = np.random.default_rng(5).permutation(len(pairs))
    install(eng, pairs=pairs[perm])
    b = call(eng, st, None, C, 1, True)
    assert b["dist"].tobytes() == np.ascontiguousarray(a["dist"][:, perm]).tobytes() and np.array_equal(b["idx"], a["idx"][:, perm])
    install(eng, meshes=list(meshes.items())[::-1])
    assert same(call(eng, st, None, C, 1, True), a)
    eng3 = _engine(topo, False, options={"hull_large_all": 1})
    install(eng3)
    c = call(eng3, st, None, C, 1, True)
    mp = is_mesh_pair(pairs, meshes)
    assert c["dist"][:, mp].tobytes() == a["dist"][:, mp].tobytes() and np.array_equal(c["idx"], a["idx"])
    eng3.set_hulls(hulls, pairs, large=True)
    plain = call(eng3, st, None, C, 1, True)
    assert c["dist"][:, ~mp].tobytes() == plain["dist"][:, ~mp].tobytes()
    for e in (eng, eng2, eng3):
        e.close()


def test_refusals_leave_the_attachments_in_place():
    from flobaroid_amd._lib import FbrError

    T = 63
    topo, hulls, meshes, pairs = gantry_set()
    st, val, idx, bar = gantry_reference(T, False)
    eng = _engine(topo, False)
    with pytest.raises(FbrError, match="code -1"):  # no hull set
        eng.set_large_hull_meshes(meshes)
    install(eng)
    a = call(eng, st, None, C, 1, True)
    t0 = meshes[0]
    for bad in ({len(hulls): t0}, [(0, t0), (0, t0)], {0: t0[:0]}, {0: t0 * 3.0}, {0: np.where(np.arange(t0.size).reshape(t0.shape) == 4, np.nan, t0)},
                {0: np.tile(t0[:1], (8193, 1, 1))}):
        with pytest.raises(FbrError, match="code -1"):
            eng.set_large_hull_meshes(bad)
    with pytest.raises(FbrError, match="fbr_model_set_hull_meshes: hull 4 of the set has 132 vertices"):  # the small call keeps its refusal
        eng.set_hull_meshes({0: t0[:100]})
    assert same(call(eng, st, None, C, 1, True), a)
    smp = np.zeros((C, len(pairs)), dtype=np.int64)
    for grad, name in ((eng.hull_distance_gradients, "fbr_hull_distance_gradients"), (eng.mesh_distance_gradients, "fbr_mesh_distance_gradients"),
                       (eng.large_hull_distance_gradients, "fbr_large_hull_distance_gradients")):
        with pytest.raises(FbrError, match=name + r": the hull set has triangle meshes attached by fbr_model_set_large_hull_meshes") as e:
            grad(st, C, smp)
        assert "code -4" in str(e.value)
    assert same(call(eng, st, None, C, 1, True), a)
    # a small hull set with a large attachment: the hull and the mesh gradient call refuse it too; cleared, the hull call serves the set
    small = [0, 1, 2, 3, 5, 6, 7]
    sub = np.array([(small.index(x), small.index(y)) for x, y in pairs if x in small and y in small], dtype=np.int32)
    eng.set_hulls([hulls[i] for i in small], sub, meshes={small.index(h): t for h, t in meshes.items() if h in small}, large_meshes=True)
    smp = np.zeros((C, len(sub)), dtype=np.int64)
    for grad in (eng.hull_distance_gradients, eng.mesh_distance_gradients):
        with pytest.raises(FbrError, match="fbr_model_set_large_hull_meshes"):
            grad(st, C, smp)
    eng.set_large_hull_meshes({})
    assert np.isfinite(_host(eng.hull_distance_gradients(st, C, smp))["dist"]).all()
    eng.close()


# ---- (g) KUKA LWR4 in collisionMode "full" ------------------------------------------------------------------------------------------------------------
def test_kuka_full_mode_collision_block_and_the_gradient_refusal():
    """Fixed base, the eight visual meshes on the hulls of their vertices (158 to 793) and the floor of world_kuka.urdf; C = 2, T = 64,
    collisionCheckStep 1, no transitions.  The block's values equal the emulation evaluated at the winning configurations (bar: 32 eps x
    the pair's scale, the smaller term of the project's rule), the indices equal the emulation's over all samples for two pairs."""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from flobaroid_amd.collision import FBR_MAX_LARGE_HULL_VERTICES, FBR_MAX_LARGE_MESH_TRIANGLES, collision_set, hulls_from_urdf, meshes_from_urdf, world_hulls_from_urdf
    from test_gpu_box_objectives import _cols

    topo = load_topo("kuka_lwr4")
    urdf = os.path.join(URDF, "kuka_lwr4.urdf")
    hulls, box_links = hulls_from_urdf(urdf, topo.link_names, max_vertices=FBR_MAX_LARGE_HULL_VERTICES)
    ms = meshes_from_urdf(urdf, list(hulls), max_triangles=FBR_MAX_LARGE_MESH_TRIANGLES)
    assert not box_links and len(ms) == 8 and max(len(m.triangles) for m in ms.values()) == 4434
    wh = world_hulls_from_urdf(os.path.join(URDF, "world_kuka.urdf"), "geometric")
    eng = Engine(topo, floating=False)
    rng = np.random.default_rng(36)
    n, T, freq = topo.num_dofs, 64, 100.0
    config = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0, "collisionCheckStep": 1,
              "transitionDuration": 0.0, "collisionMode": "full", "worldCollisionMargin": 0.01}
    posture = np.array([0.3, 1.9, -0.4, -1.2, 0.5, 0.9, 0.2])
    cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.05 for _ in range(n)], [rng.standard_normal(2) * 0.05 for _ in range(n)],
                                      posture + rng.uniform(-0.02, 0.02, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    q = _host(exc.candidate_states(eng, cands, T, freq))["q"]
    cs = collision_set(topo, {}, config, hulls=hulls, world_hulls=wh, meshes=ms, large_meshes=True)
    P = len(cs["pair_names"])
    assert cs["large_meshes"] and len(cs["meshes"]) == 8 and P >= 20, cs["pair_names"]
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    cols = _cols(eng, topo, False)
    base = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config)
    full = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, collision=cs)
    n0 = base["g"].shape[1]
    assert full["g"].shape == (C, n0 + P) and full["g"][:, :n0].tobytes() == base["g"].tobytes()
    blk, arg = full["g"][:, n0:], full["ag_cache"]["collision_argmin_idx"]
    pr = cs["hull_pairs"][cs["columns"][:, 1]]  # in the order of pair_names
    fr = frames_of(topo, cs["hulls"], q, bool(cs.get("offset_in_link_axes", False)))
    diam = np.array([h.diameter for h in cs["hulls"]])
    assert np.all(arg >= 0) and np.all(arg < T)
    worst = 0.0
    for c in range(C):
        rows = c * T + arg[c]
        for k in range(P):
            got, _ = tl.pairs_emul(fr[rows[k]:rows[k] + 1], cs["hulls"], cs["meshes"], pr[k:k + 1], True)
            a, b = pr[k]
            bar = 32.0 * EPS * (np.linalg.norm(fr[rows[k], b, 9:] - fr[rows[k], a, 9:]) + diam[a] + diam[b])
            err = abs(blk[c, k] - (got[0, 0] - cs["margins"][k]))
            worst = max(worst, err / bar)
            assert err <= bar, (c, cs["pair_names"][k], blk[c, k], got[0, 0])
    # the indices over all samples, for the wrist against the base and the flange against the second link
    two = [cs["pair_names"].index(p) if p in cs["pair_names"] else cs["pair_names"].index(p[::-1])
           for p in (("lwr_base_link", "lwr_7_link"), ("lwr_2_link", "lwr_6_link"))]
    emu, sa = tl.pairs_emul(fr, cs["hulls"], cs["meshes"], pr[two], True)
    _, eidx = hr.candidate_minimum(emu, C, 1)
    assert np.array_equal(eidx, arg[:, two])
    print(f"KUKA full: {P} pairs, block against the emulation at the winning configurations {worst:.3f} bars at most; {int((blk < 0).sum())} of {blk.size} "
          f"entries in collision or inside the margin; distances {blk.min():.4f} .. {blk.max():.4f}; the two pairs over all samples: the tree "
          f"evaluated {sa['evals']} triangle pairs, {sa['node_pairs']} node pairs")
    for kw in ({}, {"mesh_gradient": True}, {"large_hull_gradient": True}):
        with pytest.raises(ValueError, match=r"lwr_base_link \(4434 triangles on a hull of 216 vertices\)"):
            exc.candidate_gradients_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, dopt_scale=1.0, collision=cs, **kw)
    eng.close()
