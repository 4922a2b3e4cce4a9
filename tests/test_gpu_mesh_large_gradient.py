"""fbr_large_mesh_distance_gradients / Engine.large_mesh_distance_gradients and the large_mesh_gradient=True path of excitation on the device
(csrc/fbr_mesh_bvh_grad.h), on the gantry set and shapes of tests/test_gpu_meshes_large.py / tests/mesh_large_shapes.py.

The exact tests are byte equalities between two device runs: (a) a set whose meshes fit both attachments through the new call against
fbr_mesh_distance_gradients on the small attachment, C = 1, 63, 64, 65; (b) the class routes of the gantry set -- SMALL columns against
fbr_hull_distance_gradients of those pairs alone, BIG columns against fbr_large_hull_distance_gradients of the set without meshes, MESH
columns against the new call with those pairs alone; (c) option mesh_grad_order 1 and 2 against 0, host against device states, a second
run, each of the 65 candidates alone; (d) mesh_grad_order = 3 refused by name with the set left in place, and the three older calls refusing the
tree set as before.

Against the emulation (tests/emul/mesh_bvh_grad_emul.cpp: the restatement of the three stages, held bit for bit to the brute-force single
pass by tests/test_mesh_large_gradient.py) stage A's kinematics differ in the last bits between device and g++, so (e) and (f) take the bar
of tests/test_gpu_mesh_gradient.py: per entry |delta grad| <= (b+ + b-) / (2 eps), b+- = max(10 dev, 32 EPS scale), the centre distance
within max(10 dev, 32 EPS scale), entries the stencil never touches exactly 0.0, and every compared stencil value more than 100 bars from 0
(at most 1 in 10 of the (candidate, pair) entries may be left out by that rule: asserted).  dev, in that file the emulation's deviation
from the NumPy restatement, is 1.1e-16 on these shapes (tests/test_gpu_meshes_large.py measures it), a hundred times below the second
term, which therefore is the bar here: never a wider one.  (f) is KUKA LWR4 end to end, collisionMode "full" and "convex" with
fullMeshLinks.

Largest |delta grad| / bar measured on an MI355X: (e) the gantry 0.0000 in both offset modes, the centre distances to the bit (its joints are
prismatic: the device's kinematics have the emulation's bits), no entry left out; on KUKA's chain (revolute joints, 33 candidates) soup 0.0131, blob x blob 0.0112, the sphere against 129 vertices
0.0091, the torus 0.0156 with 2 of 140 entries left out, the centre distances within 0.023 bars; (f) the call's centre distances equal the
block's g + margin on all 58 entries; KUKA 0.0080 over the three pairs apart, their centre
distances within 0.006 bars, no entry left out; 3 of the 29 pairs touch as meshes (the floor against the base and links 3 and 4)."""
import functools
import os

import numpy as np
import pytest

import hull_restatement as hr
import mesh_large_shapes as ml
import test_gpu_meshes_large as gl
import test_mesh_large_gradient as tg
import test_meshes_large as tl
from common import GOLDEN, load_topo
from test_gpu_boxes import _engine
from test_gpu_meshes import is_mesh_pair
from test_hulls import EPS, as_tuples

pytestmark = pytest.mark.gpu
URDF = os.path.join(GOLDEN, "urdf")
T = 4  # samples a candidate


def _cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _same(a, b):
    return a["dist"].tobytes() == b["dist"].tobytes() and a["grad_q"].tobytes() == b["grad_q"].tobytes()


def _cols(a, sel):
    return {k: np.ascontiguousarray(v[:, sel]) for k, v in a.items()}


def gantry_q(C, seed):
    """(C T, 2): lift within [0.05, 0.3], slide within [-0.2, 0.2], the ranges of tests/test_gpu_meshes_large.py gantry_states"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([rng.uniform(0.05, 0.3, C * T), rng.uniform(-0.2, 0.2, C * T)], axis=1))


def items(C, P, seed):
    """sample with some -1 entries, a scale near 1, a pose_sample of its own"""
    rng = np.random.default_rng(seed)
    sample = rng.integers(0, T, (C, P)).astype(np.int64)
    sample[rng.random((C, P)) < 0.15] = -1
    sample[0, 0] = 0
    if C > 1:
        sample[C - 1, P - 1] = -1
    return sample, rng.uniform(0.9, 1.0, (C, P)), rng.integers(-1, T, (C, P)).astype(np.int64)


# ---- (a) small against tree ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def both_set():
    """the gantry with meshes that fit BOTH attachments: at most 256 triangles a mesh, at most 32768 triangle pairs a pair, hulls of at most
    128 vertices"""
    from flobaroid_amd.collision import Hull
    import hull_shapes as hs

    g = gl.gantry_set()
    topo, s = g[0], tl.shapes()
    hulls = [ml.hull_of(s["blob"], "bed", offset=[1.5, 0.0, 0.0]), ml.hull_of(s["soup2L1"], "carriage", offset=[1.25, 0.0, -0.05]),
             ml.hull_of(s["soupL1"], "bed", offset=[0.25, 0.0, 0.0]), ml.hull_of(s["blob2"], "carriage", offset=[0.0, 0.0, -0.35]),
             Hull("column", hs.box([0.0625, 0.0625, 0.0625]), np.array([0.0, 1.5, 0.0])), Hull("bed", hs.prism(64, 0.25, 0.5), np.array([0.25, 0.6, 0.0]))]
    meshes = {0: s["blob"], 1: s["soup2L1"], 2: s["soupL1"], 3: s["blob2"]}
    pairs = np.array([(0, 1), (2, 3), (4, 0), (3, 5), (1, 4), (4, 5), (3, 2)], dtype=np.int32)
    assert max(len(t) for t in meshes.values()) <= 256 and max(len(h.vertices) for h in hulls) <= 128
    assert max(len(meshes.get(a, [0])) * len(meshes.get(b, [0])) for a, b in pairs) <= 32768
    return topo, hulls, meshes, pairs


@pytest.mark.parametrize("C", [1, 63, 64, 65])
def test_tree_attachment_gives_the_bytes_of_the_small_attachment(C):
    topo, hulls, meshes, pairs = both_set()
    P = len(pairs)
    q = gantry_q(C, 60 + C)
    sample, scale, pose = items(C, P, 70 + C)
    assert (sample < 0).any() or C == 1
    eng = _engine(topo, False)
    st = {"q": _cuda(q)}
    eng.set_hulls(hulls, pairs, meshes=meshes)
    old = _host(eng.mesh_distance_gradients(st, C, _cuda(sample), scale=_cuda(scale), pose_sample=_cuda(pose)))
    eng.set_hulls(hulls, pairs, meshes=meshes, large_meshes=True)
    new = _host(eng.large_mesh_distance_gradients(st, C, _cuda(sample), scale=_cuda(scale), pose_sample=_cuda(pose)))
    assert _same(old, new)
    live = sample >= 0
    assert np.all(new["dist"][~live] == tg.NONE) and np.all(new["grad_q"][~live] == 0.0) and np.isfinite(new["grad_q"]).all()
    assert np.abs(new["grad_q"][live]).max() > 1e-2 and np.all(new["dist"][live & is_mesh_pair(pairs, meshes)[None, :]] >= 0.0)
    eng.close()


# ---- (b) the class routes -------------------------------------------------------------------------------------------------------------------------
def test_every_class_takes_its_own_route():
    """the gantry set of tests/test_gpu_meshes_large.py, installed with large=True: seven MESH pairs, box x prism SMALL, box x 129 vertices BIG"""
    topo, hulls, meshes, pairs = gl.gantry_set()
    C, P = 5, len(pairs)
    mp = is_mesh_pair(pairs, meshes)
    bigp = np.array([not m and max(len(hulls[a].vertices), len(hulls[b].vertices)) > 128 for m, (a, b) in zip(mp, pairs)])
    small = ~mp & ~bigp
    assert mp.sum() == 7 and bigp.sum() == 1 and small.sum() == 1
    q = gantry_q(C, 81)
    sample, scale, pose = items(C, P, 82)
    eng = _engine(topo, False)
    st = {"q": q}
    call = lambda f, sel: f(st, C, np.ascontiguousarray(sample[:, sel]), scale=np.ascontiguousarray(scale[:, sel]),  # noqa: E731
                            pose_sample=np.ascontiguousarray(pose[:, sel]))
    every = np.ones(P, dtype=bool)
    gl.install(eng)
    got = call(eng.large_mesh_distance_gradients, every)
    # SMALL: the hull call on those pairs installed alone, on a set of fbr_model_set_hulls
    used = sorted(set(pairs[small].reshape(-1)))
    eng.set_hulls([hulls[i] for i in used], np.array([(used.index(a), used.index(b)) for a, b in pairs[small]], dtype=np.int32))
    assert _same(call(eng.hull_distance_gradients, small), _cols(got, small))
    # BIG: the large-hull call on the set without meshes
    eng.set_hulls(hulls, pairs, large=True)
    assert _same(_cols(call(eng.large_hull_distance_gradients, every), bigp), _cols(got, bigp))
    # MESH: the new call with those pairs installed alone
    gl.install(eng, pairs=pairs[mp])
    assert _same(call(eng.large_mesh_distance_gradients, mp), _cols(got, mp))
    # option hull_large_all has no effect
    eng2 = _engine(topo, False, options={"hull_large_all": 1})
    gl.install(eng2)
    assert _same(call(eng2.large_mesh_distance_gradients, every), got)
    live = sample >= 0
    assert np.isfinite(got["grad_q"]).all() and np.all(got["dist"][~live] == tg.NONE) and np.all(got["dist"][live & mp[None, :]] > 0.0)
    for e in (eng, eng2):
        e.close()


# ---- (c), (d) orders, determinism, refusals ---------------------------------------------------------------------------------------------------------
def test_orders_states_runs_and_candidates_give_the_same_bytes_and_the_refusals():
    from flobaroid_amd._lib import FbrError

    topo, hulls, meshes, pairs = gl.gantry_set()
    C, P = 65, len(pairs)
    q = gantry_q(C, 91)
    sample, scale, pose = items(C, P, 92)
    eng = _engine(topo, False)
    gl.install(eng)
    a = eng.large_mesh_distance_gradients({"q": q}, C, sample, scale=scale, pose_sample=pose)
    assert isinstance(a["dist"], np.ndarray) and a["grad_q"].shape == (C, P, 2)
    assert _same(eng.large_mesh_distance_gradients({"q": q}, C, sample, scale=scale, pose_sample=pose), a)  # a second run
    d = eng.large_mesh_distance_gradients({"q": _cuda(q)}, C, _cuda(sample), scale=_cuda(scale), pose_sample=_cuda(pose))
    assert hasattr(d["dist"], "cpu") and _same(_host(d), a)
    assert eng.get_option("mesh_grad_order") == 0
    for order in (1, 2):
        eng.set_option("mesh_grad_order", order)  # (read at every call)
        assert _same(eng.large_mesh_distance_gradients({"q": q}, C, sample, scale=scale, pose_sample=pose), a), order
    # every candidate alone, in the default order and (a candidate alone in slot-major order is one stencil point a lane group) in slot-major
    for order in (0, 2):
        eng.set_option("mesh_grad_order", order)
        for c in range(C):
            rows = slice(c * T, (c + 1) * T)
            one = eng.large_mesh_distance_gradients({"q": np.ascontiguousarray(q[rows])}, 1, sample[c:c + 1], scale=scale[c:c + 1], pose_sample=pose[c:c + 1])
            assert one["dist"].tobytes() == a["dist"][c:c + 1].tobytes() and one["grad_q"].tobytes() == a["grad_q"][c:c + 1].tobytes(), (c, order)
    # (d) an order that does not exist: refused by name, the set stays in place
    eng.set_option("mesh_grad_order", 3)
    with pytest.raises(FbrError, match=r"code -1.*fbr_large_mesh_distance_gradients: option mesh_grad_order"):
        eng.large_mesh_distance_gradients({"q": q}, C, sample, scale=scale, pose_sample=pose)
    eng.set_option("mesh_grad_order", 0)
    assert _same(eng.large_mesh_distance_gradients({"q": q}, C, sample, scale=scale, pose_sample=pose), a)
    for bad in (0.0, -1e-7, float("nan")):
        with pytest.raises(FbrError, match=r"code -1.*fbr_large_mesh_distance_gradients: epsilon"):
            eng.large_mesh_distance_gradients({"q": q}, C, sample, epsilon=bad)
    # the three older calls keep refusing the tree set, with the messages they had
    for grad, name in ((eng.hull_distance_gradients, "fbr_hull_distance_gradients"), (eng.mesh_distance_gradients, "fbr_mesh_distance_gradients"),
                       (eng.large_hull_distance_gradients, "fbr_large_hull_distance_gradients")):
        with pytest.raises(FbrError, match=name + r": the hull set has triangle meshes attached by fbr_model_set_large_hull_meshes: distances only") as e:
            grad({"q": q}, C, sample)
        assert "code -4" in str(e.value)
    assert _same(eng.large_mesh_distance_gradients({"q": q}, C, sample, scale=scale, pose_sample=pose), a)
    # no tree attachment: refused by the names of the calls that serve the set; no set: refused
    eng.set_hulls(hulls, pairs, large=True)
    with pytest.raises(FbrError, match=r"code -1.*fbr_mesh_distance_gradients.*fbr_large_hull_distance_gradients.*fbr_hull_distance_gradients"):
        eng.large_mesh_distance_gradients({"q": q}, C, sample)
    eng.set_hulls([], np.zeros((0, 2), dtype=np.int32))
    with pytest.raises(FbrError, match=r"code -1.*no hull set"):
        eng.large_mesh_distance_gradients({"q": q}, C, np.zeros((C, 0), dtype=np.int64))
    eng.close()


# ---- (e) against the emulation ------------------------------------------------------------------------------------------------------------------------
def held_to_the_emulation(case, C, sample, scale, got, mode, why, cols=None):
    """The bar of tests/test_gpu_mesh_gradient.py on the MESH columns ``cols`` of the device's result ``got`` ((C, P) / (C, P, n), P the
    pairs of ``case``) against the tree emulation; returns (largest |delta grad| / bar, largest |delta dist| / bar, share of the entries
    the 100-bar rule leaves out)."""
    topo, pairs, eps = case["topo"], np.asarray(case["pairs"]), 1e-7
    cols = np.arange(len(pairs)) if cols is None else np.asarray(cols)
    sub = pairs[cols]
    smp, sc = sample[:, cols], scale[:, cols]
    ed, eg, ns, stats = tg.tree_evaluate(case, C, smp, sc, None, eps, mode, route=2, pairs=sub)
    sten = stats["stencil"].reshape(C, len(cols), -1)
    Tn = case["q"].shape[0] // C
    rq = ((np.arange(C) * Tn)[:, None] + np.maximum(smp, 0)).reshape(-1)
    R, cen = hr.hull_world(topo, as_tuples(topo, case["hulls"]), case["q"][rq] * sc.reshape(-1, 1), False, None, None, mode)
    diam = np.array([h.diameter for h in case["hulls"]])
    ia, ib = np.tile(sub[:, 0], C), np.tile(sub[:, 1], C)
    rows = np.arange(C * len(cols))
    b = (32.0 * EPS * (np.linalg.norm(cen[rows, ib] - cen[rows, ia], axis=1) + diam[ia] + diam[ib])).reshape(C, len(cols))
    live = smp >= 0
    # every compared stencil value more than 100 bars from 0
    clear = live & np.all(np.isnan(sten) | (np.abs(sten) > 100.0 * b[..., None]), axis=2)
    share = 1.0 - clear.sum() / max(live.sum(), 1)
    assert share <= 0.1, (why, share)
    gd, gg = got["dist"][:, cols], got["grad_q"][:, cols]
    assert np.all(gd[~live] == tg.NONE) and np.all(gg[~live] == 0.0) and np.all(ed[~live] == tg.NONE), why
    errd = np.abs(gd - ed)[clear] / b[clear]
    errg = (np.abs(gg - eg) / ((b + b) / (2.0 * eps))[..., None])[clear]
    ev = _evaluated(case, sub, mode)
    print(f"{why}: {int(clear.sum())} of {int(live.sum())} entries compared ({share:.1%} left out by the 100-bar rule); max |delta dist| / bar = "
          f"{errd.max():.3f}, max |delta grad| / bar = {errg.max():.4f}; max |grad| = {np.abs(eg[clear]).max():.3f}; smallest stencil value "
          f"{np.nanmin(np.abs(sten[clear])):.3e}")
    assert np.all(errd <= 1.0) and np.all(errg <= 1.0), why
    # entries the stencil never touches: exactly 0.0 (a joint that moves neither member against the other has no stencil point)
    assert np.all(gg[:, ~ev] == 0.0) and np.all(eg[:, ~ev] == 0.0) and (~ev).any(), why
    return float(errg.max()), float(errd.max()), float(share)


def _evaluated(case, pairs, mode):
    """(P, n) bool: the joints whose stencil points a pair has -- the revolute and prismatic joints between its links, and in world axes the
    revolute joints above both"""
    import mesh_gradient_restatement as mg

    tup = as_tuples(case["topo"], case["hulls"])
    return np.array([mg.path_dofs(case["topo"], tup[a][0], tup[b][0], mode) for a, b in pairs])


@pytest.mark.parametrize("mode", [False, True], ids=["world-axes", "link-axes"])
def test_device_matches_the_tree_emulation_on_the_gantry(mode):
    topo, hulls, meshes, pairs = gl.gantry_set()
    C, P = 5, len(pairs)
    mp = np.nonzero(is_mesh_pair(pairs, meshes))[0]
    q = gantry_q(C, 101)
    sample, scale, pose = items(C, P, 102)
    eng = _engine(topo, False)
    eng.set_hulls(hulls, pairs, offset_in_link_axes=mode, large=True, meshes=meshes, large_meshes=True)
    got = eng.large_mesh_distance_gradients({"q": q}, C, sample, scale=scale, pose_sample=pose)
    case = {"topo": topo, "hulls": hulls, "meshes": meshes, "pairs": pairs, "q": q}
    on = _evaluated(case, pairs, mode)
    assert np.all(got["grad_q"][:, ~on] == 0.0)
    held_to_the_emulation(case, C, sample, scale, got, mode, f"gantry mode {int(mode)}", cols=mp)
    eng.close()


CHAIN = [("soup2L1", False), ("blob x blob", False), ("sphere on 132 vertices x 129 vertices", True), ("torus", True)]


def chain_inputs(kind, mode, C=33):
    """the shapes of tests/test_mesh_large_gradient.py chain_case on KUKA's chain (lwr_2_link against lwr_5_link: revolute joints only) and
    against the far world box, both orders of the members; C candidates of T configurations about the posture of that file"""
    case = tg.chain_case(kind, mode)
    pairs = np.array([(0, 1), (1, 0), (0, 3), (3, 0)] + ([(1, 3)] if 1 in case["meshes"] else []), dtype=np.int32)
    rng = np.random.default_rng(120 + tg.KINDS.index(kind))
    q = np.ascontiguousarray(tg.POSTURE + rng.uniform(-0.3, 0.3, (C * T, 7)))
    return dict(case, pairs=pairs, q=q), C, items(C, len(pairs), 130 + tg.KINDS.index(kind))


@pytest.mark.parametrize("kind,mode", CHAIN, ids=[f"{k}-{'link' if m else 'world'}-axes" for k, m in CHAIN])
def test_device_matches_the_tree_emulation_on_kukas_chain(kind, mode):
    """revolute joints, where the device's kinematics and g++'s differ in the last bits: 33 candidates x 4 or 5 pairs under the bar"""
    case, C, (sample, scale, pose) = chain_inputs(kind, mode)
    eng = _engine(case["topo"], False)
    large = max(len(h.vertices) for h in case["hulls"]) > 128
    eng.set_hulls(case["hulls"], case["pairs"], offset_in_link_axes=mode, meshes=case["meshes"], large_meshes=True, **({"large": True} if large else {}))
    got = eng.large_mesh_distance_gradients({"q": case["q"]}, C, sample, scale=scale, pose_sample=pose)
    held_to_the_emulation(case, C, sample, scale, got, mode, f"KUKA's chain, {kind}, mode {int(mode)}")
    eng.close()


# ---- (f) KUKA LWR4 end to end ---------------------------------------------------------------------------------------------------------------------------
def test_kuka_full_mode_jacobian_and_full_mesh_links():
    """The set of tests/test_gpu_meshes_large.py test_kuka_full_mode_collision_block_and_the_gradient_refusal: fixed base, C = 2, T = 64,
    collisionCheckStep 1, no transitions."""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from flobaroid_amd.collision import FBR_MAX_LARGE_HULL_VERTICES, FBR_MAX_LARGE_MESH_TRIANGLES, collision_set, hulls_from_urdf, meshes_from_urdf, world_hulls_from_urdf
    from test_gpu_box_objectives import _cols as icols_of

    topo = load_topo("kuka_lwr4")
    urdf = os.path.join(URDF, "kuka_lwr4.urdf")
    hulls, _ = hulls_from_urdf(urdf, topo.link_names, max_vertices=FBR_MAX_LARGE_HULL_VERTICES)
    ms = meshes_from_urdf(urdf, list(hulls), max_triangles=FBR_MAX_LARGE_MESH_TRIANGLES)
    wh = world_hulls_from_urdf(os.path.join(URDF, "world_kuka.urdf"), "geometric")
    eng = Engine(topo, floating=False)
    rng = np.random.default_rng(36)
    n, C, Tn, freq = topo.num_dofs, 2, 64, 100.0
    config = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0, "collisionCheckStep": 1,
              "transitionDuration": 0.0, "collisionMode": "full", "worldCollisionMargin": 0.01, "analyticalGradientEpsilon": 1e-7}
    posture = np.array([0.3, 1.9, -0.4, -1.2, 0.5, 0.9, 0.2])
    cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.05 for _ in range(n)], [rng.standard_normal(2) * 0.05 for _ in range(n)],
                                      posture + rng.uniform(-0.02, 0.02, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    q = _host(exc.candidate_states(eng, cands, Tn, freq))["q"]
    cs = collision_set(topo, {}, config, hulls=hulls, world_hulls=wh, meshes=ms, large_meshes=True)
    names, P = cs["pair_names"], len(cs["pair_names"])
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    args = (eng, cands, Tn, freq, topo.x_std(), icols_of(eng, topo, False), limits, topo.dof_names, config)
    full = exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0, collision=cs, large_mesh_gradient=True)
    n0 = full["layout"]["collision"]
    assert full["g"].shape == (C, n0 + P) and all(v.shape[1] == n0 + P for v in full["con_grad"].values())
    coll = exc.candidate_collision_gradient_from_coefficients(eng, cands, Tn, freq, config, cs, large_mesh_gradient=True)
    assert np.array_equal(coll["g"], full["g"][:, n0:]) and coll["grad_q"].shape == (C, P, n)
    for k, v in coll["grad"].items():
        assert np.array_equal(full["con_grad"][k][:, n0:], v), k
    rows = coll["grad_q"]
    assert np.isfinite(rows).all() and all(np.isfinite(v).all() for v in full["con_grad"].values())
    # every row is zero outside the joints between its two links
    pr = cs["hull_pairs"][cs["columns"][:, 1]]  # in the order of pair_names
    mode = bool(cs.get("offset_in_link_axes", False))
    case = {"topo": topo, "hulls": cs["hulls"], "meshes": cs["meshes"], "pairs": pr, "q": q}
    on = _evaluated(case, pr, mode)
    assert np.all(rows[:, ~on] == 0.0) and (~on).any() and np.abs(rows).max() > 1e-2
    # four pairs against the tree emulation: the wrist and the base, the flange and link 2, a link and the ground, one that touches
    st = exc.candidate_states(eng, cands, Tn, freq, device=True)
    cons = exc._collision_block(eng, st, C, config, cs)
    at = lambda a, b: names.index((a, b)) if (a, b) in names else names.index((b, a))  # noqa: E731
    margins = np.asarray(cs["margins"], dtype=np.float64)
    touching = [k for k in range(P) if np.all(np.asarray(cons["g"])[:, k] + margins[k] == 0.0)]
    assert touching, "no pair touches as meshes: the set of the distance test has some (its block prints them)"
    ground = [k for k, (a, b) in enumerate(names) if "ground_link" in (a, b)][-1]
    four = [at("lwr_base_link", "lwr_7_link"), at("lwr_2_link", "lwr_6_link"), ground, touching[0]]
    smp, sc = np.asarray(cons["eval_sample"]), np.asarray(cons["eval_scale"])
    # the call's own centre distances at the block's evaluation points (the block has left the set installed), ALL C x P entries: within
    # 32 EPS x the pair's scale of the block's g + margin, exactly 0.0 where the pair touches; its rows are those of the layers above
    sel = np.argsort(np.asarray(cs["columns"])[:, 1], kind="stable")  # the set's own pair order
    own = lambda key: np.ascontiguousarray(np.asarray(cons[key])[:, sel])  # noqa: E731
    dg = _host(eng.large_mesh_distance_gradients(st, C, own("eval_sample"), scale=own("eval_scale"), pose_sample=own("eval_pose"), epsilon=1e-7))
    dist, gq = np.zeros((C, P)), np.zeros((C, P, n))
    dist[:, sel], gq[:, sel] = dg["dist"], dg["grad_q"]
    assert gq.tobytes() == np.ascontiguousarray(rows).tobytes()
    assert np.all(smp >= 0) and np.all(sc == 1.0)
    qw = q.reshape(C, Tn, n)[np.arange(C)[:, None], smp].reshape(C * P, n)
    _, cen = hr.hull_world(topo, as_tuples(topo, cs["hulls"]), qw, False, None, None, mode)
    diam = np.array([h.diameter for h in cs["hulls"]])
    ia, ib, at_row = np.tile(pr[:, 0], C), np.tile(pr[:, 1], C), np.arange(C * P)
    dbar = (32.0 * EPS * (np.linalg.norm(cen[at_row, ib] - cen[at_row, ia], axis=1) + diam[ia] + diam[ib])).reshape(C, P)
    block = np.asarray(cons["g"]) + margins[None, :]
    derr = np.abs(dist - block) / dbar
    print(f"KUKA full: the call's centre distances against the block's g + margin over {C * P} entries: {derr.max():.3f} bars at most")
    assert np.all(derr <= 1.0) and np.all(dist[:, touching] == 0.0) and np.all(dist >= 0.0)
    got = {"dist": dist, "grad_q": rows}
    free = [k for k in four[:3] if k not in touching]
    assert len(free) == 3, "one of the three chosen pairs touches: choose another"
    held_to_the_emulation(case, C, smp, sc, got, mode, "KUKA full, three pairs", cols=free)
    k = touching[0]
    ed, eg, _, _ = tg.tree_evaluate(case, C, smp[:, [k]], sc[:, [k]], None, 1e-7, mode, route=1, pairs=pr[[k]])
    assert np.all(ed == 0.0) and not eg.any() and np.all(got["dist"][:, k] == 0.0) and not rows[:, k].any(), names[k]
    print(f"KUKA full: {P} pairs, {len(touching)} touch as meshes ({[names[i] for i in touching]}); max |row| = {np.abs(rows).max():.3f}")
    # "convex" with fullMeshLinks: the BIG columns have the bytes of large_hull_gradient=True on the set without the mesh
    conv = dict(config, collisionMode="convex")
    fml = dict(conv, fullMeshLinks=["lwr_7_link"])
    cs7 = collision_set(topo, {}, fml, hulls=hulls, world_hulls=wh, meshes={"lwr_7_link": ms["lwr_7_link"]}, large_meshes=True)
    cs0 = collision_set(topo, {}, conv, hulls=hulls, world_hulls=wh)
    assert cs7["pair_names"] == cs0["pair_names"] == names and len(cs7["meshes"]) == 1
    a7 = exc.candidate_collision_gradient_from_coefficients(eng, cands, Tn, freq, fml, cs7, large_mesh_gradient=True)
    a0 = exc.candidate_collision_gradient_from_coefficients(eng, cands, Tn, freq, conv, cs0, large_hull_gradient=True)
    big = np.array(["lwr_7_link" not in p for p in names])
    assert big.any() and not big.all()
    # (a row is the gradient at the block's winning configuration: the BIG columns' distances, hence their winners, are the same in both sets)
    assert np.ascontiguousarray(a7["g"][:, big]).tobytes() == np.ascontiguousarray(a0["g"][:, big]).tobytes()
    assert np.ascontiguousarray(a7["grad_q"][:, big]).tobytes() == np.ascontiguousarray(a0["grad_q"][:, big]).tobytes()
    assert np.isfinite(a7["grad_q"]).all() and np.all(a7["g"][:, ~big] >= a0["g"][:, ~big] - 1e-12)
    eng.close()
