"""The hull distance gradient off the GPU: the HIP-free text of csrc/fbr_hull_grad.h (g++, tests/emul/hull_grad_emul.cpp: one walk, rigidly
moved hulls, evaluated joints only, GJK and the facet pass) against the NumPy / Qhull restatement (tests/hull_gradient_restatement.py: whole
re-walks, every joint, the Minkowski difference handed to Qhull); contacts of known slope on the gantry of tests/hull_shapes.py; the
restatement against a Richardson-extrapolated central difference of wider steps; the hull_gradient=True path of
excitation.candidate_collision_gradient against a stub engine; the new symbol in header, binding and library.

Measured here (g++ 13, x86-64), largest |emulation - restatement| / bar per robot over both offset modes and both steps: threeLinks
0.018, kuka_lwr4 0.051, walkman_left_arm 0.032, random tree 0.025; the 128-vertex pair on the gantry 0.003.  Three edits of a scratch copy
of csrc/fbr_box_grad.h (fbr_rigidgrad_item) were each caught by the emulation tests here: without the world-axes "above both links"
branch 4 tests fail, with B moved where A should move 21, with sg = +1 for both stencil points all 22."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hull_gradient_restatement as hg
import hull_restatement as hr
import hull_shapes as hs
from common import ROOT, load_topo, random_states, random_topology
from test_box_gradient import ROBOTS, T, item_arrays
from test_boxes import mixed_pairs, synthetic_boxes, world_boxes_near
from test_hulls import _c, _p, as_tuples, link_index, tables

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "hull_grad_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libhull_grad_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_lib = None


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC, os.path.join(ROOT, "include", "fbr.h")] + [os.path.join(_CSRC, h) for h in (
            "fbr_hull_grad.h", "fbr_hull.h", "fbr_box_grad.h", "fbr_box.h", "fbr_capsule_grad.h", "fbr_capsule.h", "fbr_math.h", "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


def emul_items(topo, floating, hulls, item_pairs, q, rpy, base_pos, mode, eps):
    """(dist (M,), grad (M, n)) of one hull pair per configuration from the library's own walk, item routine and hull distance on the CPU;
    ``hulls``: flobaroid_amd.collision.Hull objects"""
    parent, dof, jt = _c(topo.parent, np.int32), _c(topo.dof_index, np.int32), _c(topo.joint_type, np.int32)
    rR, rp, ax = _c(topo.rest_R).reshape(-1), _c(topo.rest_p).reshape(-1), _c(topo.axis).reshape(-1)
    link = _c(link_index(topo, hulls), np.int32)
    off = _c([h.offset for h in hulls]).reshape(-1)
    rot = _c([np.eye(3) if h.rot is None else h.rot for h in hulls]).reshape(-1)
    vbeg, v, fbeg, pl, ebeg, ed, _ = tables(hulls)
    pr = _c(item_pairs, np.int32).reshape(-1)
    q = _c(q)
    M = q.shape[0]
    rpy = None if rpy is None or not floating else _c(rpy)
    bp = None if base_pos is None or not floating else _c(base_pos)
    dist, grad = np.zeros(M), np.full((M, topo.num_dofs), np.nan)
    rc = emul().hullgrad_eval(topo.num_links, topo.num_dofs, _p(parent), _p(dof), _p(rR), _p(rp), _p(ax), _p(jt), int(floating), len(hulls), _p(link),
                              _p(off), _p(rot), int(mode), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), ctypes.c_double(eps), ctypes.c_long(M),
                              _p(pr), _p(q), _p(rpy), _p(bp), _p(dist), _p(grad))
    assert rc == 0
    return dist, grad


def emul_evaluate(case, C, sample, scale, pose, eps, mode, pairs=None):
    """the contract of fbr_hull_distance_gradients from the emulation: (dist (C, P), grad (C, P, n))"""
    topo, fl = case["topo"], case["floating"]
    pairs = case["pairs"] if pairs is None else pairs
    P, Tn = len(pairs), case["q"].shape[0] // C
    sample = np.asarray(sample).reshape(C, P)
    ps = sample if pose is None else np.where(np.asarray(pose) < 0, sample, pose)
    sc = np.ones((C, P)) if scale is None else np.asarray(scale)
    base = (np.arange(C) * Tn)[:, None]
    rq, rp = (base + np.maximum(sample, 0)).reshape(-1), (base + np.maximum(ps, 0)).reshape(-1)
    dist, grad = emul_items(topo, fl, case["hulls"], np.tile(pairs, (C, 1)), case["q"][rq] * sc.reshape(-1, 1), case["rpy"][rp] if fl else None,
                            case["bp"][rp] if fl else None, mode, eps)
    none = sample < 0
    return np.where(none, hg.NONE, dist.reshape(C, P)), np.where(none[..., None], 0.0, grad.reshape(C, P, -1))


# ---- the cases (shared with tests/test_gpu_hull_gradient.py) ----------------------------------------------------------------------------------
def small_hull(rng, kind, link_name, half, offset, rot=None, name=None):
    """kind 0: a tetrahedron; 1: the box of these half extents (hull_from_box); 2: 12 random points on the ellipsoid of these semi-axes --
    4, 8 and 12 vertices, so that the Qhull restatement of a test stays at a few seconds"""
    from flobaroid_amd.collision import Box, Hull, hull_from_box

    if kind == 1:
        return hull_from_box(Box(link_name, half, offset, rot, name))
    if kind == 0:
        pts = rng.standard_normal((4, 3)) * half
    else:
        pts = rng.standard_normal((12, 3))
        pts = pts / np.linalg.norm(pts, axis=1, keepdims=True) * half
    return Hull(link_name, pts, offset, rot, name)


def make_case(robot, C=5, max_pairs=16):
    """robot, a small hull on every link (of the size of test_boxes.synthetic_boxes, the three kinds in turn) and three world hulls near
    the links (world_boxes_near), the pairs of test_boxes.mixed_pairs with every second world pair turned round (the world hull first),
    at most ``max_pairs`` of them, C candidates of T = 7 samples"""
    floating, seed = ROBOTS[robot]
    rng = np.random.default_rng(seed)
    rnd = robot == "random"
    topo = random_topology(rng, 9, p_fixed=0.25, branchiness=0.5, p_prismatic=0.3) if rnd else load_topo(robot)
    assert not rnd or {0, 1, 2} <= set(topo.joint_type[1:]), "the random tree needs fixed, revolute and prismatic joints: change the seed"
    boxes = synthetic_boxes(topo, rng, pad=(0.2, 0.6)) if rnd else synthetic_boxes(topo, rng)
    S = C * T
    st = random_states(topo, S, rng, floating, use_limits=not rnd)
    rpy = rng.uniform(-0.6, 0.6, (S, 3)) if floating else None
    bp = rng.standard_normal((S, 3)) * 0.1 if floating else None
    import box_restatement as br

    _, p = br.link_poses(topo, st["q"], floating, rpy, bp)
    boxes = boxes + (world_boxes_near(rng, np.concatenate([x for x in p]), 3, half=(0.3, 0.8)) if rnd else
                     world_boxes_near(rng, np.concatenate([x for x in p]), 3))
    pairs = mixed_pairs(topo, boxes)
    wp = np.nonzero(np.array([boxes[b][0] < 0 for _, b in pairs]))[0]
    pairs[wp[::2]] = pairs[wp[::2], ::-1]
    if max_pairs is not None and len(pairs) > max_pairs:
        pairs = pairs[np.sort(rng.choice(len(pairs), max_pairs, replace=False))]
    hulls = [small_hull(rng, i % 3, topo.link_names[l] if l >= 0 else None, h, c, R, None if l >= 0 else f"world{i}") for i, (l, h, c, R) in enumerate(boxes)]
    return {"robot": robot, "topo": topo, "floating": floating, "hulls": hulls, "tuples": as_tuples(topo, hulls), "pairs": np.ascontiguousarray(pairs),
            "q": st["q"], "rpy": rpy, "bp": bp, "C": C, "seed": seed}


_CASES = {}


def case_of(robot):
    if robot not in _CASES:
        _CASES[robot] = make_case(robot)
    return _CASES[robot]


def reference(case, C, pairs, sample, scale, pose, eps, mode):
    """the restatement with the bar for the emulation's deviation on the same items: (ref, emulated dist, emulated grad)"""
    ref = hg.evaluate(case["topo"], case["tuples"], pairs, case["floating"], case["q"], case["rpy"], case["bp"], C, sample, scale, pose, eps, mode)
    ed, eg = emul_evaluate(case, C, sample, scale, pose, eps, mode, pairs)
    fin = np.isfinite(ref["dist"])
    assert np.array_equal(fin, np.isfinite(ed))
    dev = float(np.abs(ed - ref["dist"])[fin & ~ref["none"]].max())
    return hg.with_dev(ref, dev), ed, eg


@pytest.mark.parametrize("eps", [1e-7, 1e-4])
@pytest.mark.parametrize("mode", [False, True], ids=["world-axes", "link-axes"])
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_library_text_equals_the_restatement(robot, mode, eps):
    """the g++ build of fbr_hullgrad_item within ``bar`` of the restatement entry by entry, the distance within the distance bar, joints the
    stencil never touches exactly 0.0; both signs occur among the centre distances (asserted before the comparison)"""
    case = case_of(robot)
    C, P = case["C"], len(case["pairs"])
    rng = np.random.default_rng(11)
    for with_scale in (False, True):
        sample, scale, pose = item_arrays(case, rng, C, P, with_scale)
        ref, ed, eg = reference(case, C, case["pairs"], sample, scale, pose, eps, mode)
        live = ~ref["none"]
        assert (ref["dist"][live] > 0).any() and (ref["dist"][live] <= 0).any(), "the centre distances need both signs: change the case"
        worst = (np.abs(eg - ref["grad"]) / ref["bar"]).max()
        print(f"{robot} mode {int(mode)} eps {eps:g} scale {with_scale}: P = {P}, separated {100 * (ref['dist'][live] > 0).mean():.0f} %, "
              f"max |delta grad| / bar = {worst:.3f}, max |grad| = {np.abs(ref['grad']).max():.3f}")
        assert np.all(np.abs(ed - ref["dist"])[live] <= ref["dist_bar"][live]) and np.all(ed[~live] == hg.NONE)
        assert np.all(np.abs(eg - ref["grad"]) <= ref["bar"])
        assert np.all(eg[~ref["on_path"]] == 0.0) and np.all(eg[~live] == 0.0)
        assert ref["on_path"].any() and np.abs(ref["grad"]).max() > 1e-2
        # the world hull is the first member of some pairs and the second of others
        first = np.array([case["tuples"][a][0] < 0 for a, _ in case["pairs"]])
        second = np.array([case["tuples"][b][0] < 0 for _, b in case["pairs"]])
        assert first.any() and second.any()


def test_library_text_corner_rules():
    """two hulls on one link: a zero row and a finite distance; a NaN configuration: NaN in the distance and the evaluated joints, exact
    zeros elsewhere"""
    case = case_of("kuka_lwr4")
    topo, hulls = case["topo"], list(case["hulls"])
    hulls.append(small_hull(np.random.default_rng(2), 0, hulls[4].link_name, np.array([0.05, 0.04, 0.03]), np.array([0.3, 0.0, 0.1])))
    q = case["q"][:1]
    dist, grad = emul_items(topo, False, hulls, [[4, len(hulls) - 1], [1, 6]], np.repeat(q, 2, axis=0), None, None, True, 1e-7)
    assert np.all(grad[0] == 0.0) and np.isfinite(dist[0]) and np.abs(grad[1]).max() > 0
    qn = q.copy()
    qn[0, 2] = np.nan
    dist, grad = emul_items(topo, False, hulls, [[1, 6]], qn, None, None, True, 1e-7)
    tup = as_tuples(topo, hulls)
    on = hg.path_dofs(topo, tup[1][0], tup[6][0])
    assert np.isnan(dist[0]) and np.all(np.isnan(grad[0][on])) and np.all(grad[0][~on] == 0.0) and (~on).any()


# ---- the gantry: contacts of known slope ------------------------------------------------------------------------------------------------------
def gantry_case(kind, gap=0.0):
    """The gantry of tests/hull_shapes.py (DOF 0 lifts along z, DOF 1 slides along x; exact poses) with hulls whose distance has a known
    slope.  "stack": a box on the bed (its top at z = 0.125), a smaller box on the carriage whose bottom is ``gap`` above that top and whose
    footprint lies inside it, and a world box whose bottom is ``gap`` above the carriage box's top; pairs (bed, carriage), (carriage, bed),
    (carriage, world), (world, carriage).  "round": the 128-point sphere on the carriage inside the reach of the 64-gon prism on the bed and
    of the same prism as a turned world hull: the largest tables."""
    from flobaroid_amd.collision import Box, Hull, hull_from_box

    topo = hs.gantry()
    if kind == "stack":
        hulls = [hull_from_box(Box("bed", np.array([0.25, 0.25, 0.125]), np.zeros(3))),
                 hull_from_box(Box("carriage", np.array([0.125, 0.125, 0.125]), np.zeros(3))),
                 hull_from_box(Box(None, np.array([0.25, 0.25, 0.125]), np.array([0.0, 0.0, 0.5 + 2.0 * gap]), np.eye(3), "lid"))]
        q = np.array([[-0.25 + gap, -0.25]])  # the carriage's origin at (0, 0, 0.25 + gap)
    else:
        hulls = [Hull("bed", hs.prism(64, 0.25, 0.3), np.zeros(3)), Hull("carriage", hs.fibonacci_sphere(128, 0.25), np.zeros(3)),
                 Hull(None, hs.prism(64, 0.25, 0.3), np.array([0.3, 0.1, 0.6]), hs.TURNS["quarter"], "lid")]
        q = np.array([[-0.2, -0.1]])  # the sphere's centre at (0.15, 0, 0.3): 0.1 deep in the prism on the bed, and in the turned one above
    pairs = np.array([[0, 1], [1, 0], [1, 2], [2, 1]], dtype=np.int32)
    return {"robot": "gantry", "topo": topo, "floating": False, "hulls": hulls, "tuples": as_tuples(topo, hulls), "pairs": pairs, "q": q, "rpy": None,
            "bp": None, "C": 1}


STACK_ROWS = np.array([[1.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [-1.0, 0.0]])  # lifting opens the lower gap and closes the upper one


@pytest.mark.parametrize("mode", [False, True], ids=["world-axes", "link-axes"])
@pytest.mark.parametrize("gap", [1e-2, -1e-3], ids=["apart", "deep"])
def test_gantry_stacked_hulls_have_unit_rows(gap, mode):
    """parallel faces stacked along the lift axis, 1e-2 apart (GJK) and 1e-3 deep (the facet pass): the distance is the gap, its row +-1 in
    the lift and 0 in the slide, within the bar, in the emulation and in the restatement"""
    case = gantry_case("stack", gap)
    smp = np.zeros((1, 4), dtype=np.int64)
    for eps in (1e-7, 1e-4):
        ref, ed, eg = reference(case, 1, case["pairs"], smp, None, None, eps, mode)
        assert np.all(np.abs(ed[0] - gap) <= ref["dist_bar"][0]) and np.all(np.abs(ref["dist"][0] - gap) <= ref["dist_bar"][0])
        assert np.all(np.abs(eg[0] - STACK_ROWS) <= ref["bar"][0]) and np.all(np.abs(ref["grad"][0] - STACK_ROWS) <= ref["bar"][0])
        assert ref["on_path"][0].all() and np.all(ref["bar"] < 1e-3)


def test_gantry_sphere_in_prism_at_the_vertex_cap():
    """128 vertices against 128, overlapping: the facet pass over the largest tables, the moved copies of either member"""
    case = gantry_case("round")
    assert [len(h.vertices) for h in case["hulls"]] == [128, 128, 128]
    smp = np.zeros((1, 4), dtype=np.int64)
    for mode in (False, True):
        ref, ed, eg = reference(case, 1, case["pairs"], smp, None, None, 1e-7, mode)
        print(f"sphere in prism, mode {int(mode)}: dist {ref['dist'][0]}, max |delta grad| / bar = {(np.abs(eg - ref['grad']) / ref['bar']).max():.3f}")
        assert np.all(ref["dist"] < -1e-2)
        assert np.all(np.abs(ed - ref["dist"]) <= ref["dist_bar"]) and np.all(np.abs(eg - ref["grad"]) <= ref["bar"])
        assert np.abs(ref["grad"]).max() > 0.1


# ---- the restatement's own yardstick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["kuka_lwr4", "walkman_left_arm"])
def test_restatement_against_richardson_extrapolation(robot):
    """Along single joints, the restatement at eps = 1e-4 against (4 D(h/2) - D(h)) / 3 of central differences D of the restated distance at
    h = 1e-3 -- nothing of the stencil shared with the device.  Only entries whose three distances at 0, +-h are all positive are compared:
    the separated distance is C1, so no facet switch puts a kink there.  Its second derivative still jumps where the closest features
    change, so the bar comes from the spread |D(h) - D(h/2)| of the same entries: ten times its 99th percentile.  Entries whose spread
    exceeds the bar straddle such a jump and are left out (at most 2 %, asserted).  The g++ build of the library's text at eps = 1e-4 is
    held against the same extrapolation under the sum of that bar and its own.
    Measured: max |restatement - Richardson| = 3.1e-9 under a bar of 1.8e-6 (kuka, 230 entries), 5.1e-9 under 1.7e-6 (walkman, 290
    entries); no entry left out."""
    case = case_of(robot)
    C, P = case["C"], len(case["pairs"])
    rng = np.random.default_rng(6)
    sample, scale, pose = item_arrays(case, rng, C, P, True)
    args = (case["topo"], case["tuples"], case["pairs"], case["floating"], case["q"], case["rpy"], case["bp"], C, sample, scale, pose)
    ref, _, eg = reference(case, C, case["pairs"], sample, scale, pose, 1e-4, True)
    h = 1e-3
    Dh, Dh2 = hg.evaluate(*args, h, True), hg.evaluate(*args, h / 2, True)
    rich = (4.0 * Dh2["grad"] - Dh["grad"]) / 3.0
    use = hg.separated(Dh) & ref["on_path"]
    spread = np.abs(Dh["grad"] - Dh2["grad"])
    bar = 10.0 * np.percentile(spread[use], 99)
    smooth = use & (spread <= bar)
    err = np.abs(ref["grad"] - rich)[smooth]
    print(f"{robot}: {int(use.sum())} entries, spread 99th percentile {bar / 10:.2e}, max {spread[use].max():.2e}; left out "
          f"{100 * (1 - smooth.sum() / use.sum()):.2f} %; max |restatement - Richardson| = {err.max():.2e}, bar {bar:.2e}")
    assert use.sum() >= 100 and smooth.sum() >= 0.98 * use.sum()
    assert err.max() <= bar
    # the library's text at the same step against the same yardstick: the two bars add
    assert np.all(np.abs(eg - rich)[smooth] <= bar + ref["bar"][smooth])


# ---- the end-to-end case (shared with tests/test_gpu_hull_gradient.py) ------------------------------------------------------------------------
E2E_SEED = 4
E2E_STEP = 1e-6       # of the central difference in the optimiser's variables
E2E_FD_BAR = 5e-8     # ten times what the restatement alone gives (test_end_to_end_seed_with_the_restatement_alone: 4.2e-9), rounded up
E2E_MAX_EXCLUDED = 0.25


def e2e_case(seed=E2E_SEED):
    """kuka_lwr4 with a box hull on every link (test_boxes.synthetic_boxes) and the floor of world_kuka.urdf lifted among them, 3
    candidates of 60 samples at 20 Hz, transitions on.  Some links are left out of the check to keep the Qhull restatement of the block at
    a few seconds."""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd.collision import Box, collision_set, hull_from_box, world_hulls_from_urdf
    from common import GOLDEN

    rng = np.random.default_rng(seed)
    topo = load_topo("kuka_lwr4")
    names = topo.link_names
    hulls = {names[l]: hull_from_box(Box(names[l], h, c)) for l, h, c, _ in synthetic_boxes(topo, rng)}
    wh = world_hulls_from_urdf(os.path.join(GOLDEN, "urdf", "world_kuka.urdf"), "geometric")
    wh["ground_link"].offset = wh["ground_link"].offset + np.array([0.0, 0.0, 0.25])
    n, C, Tn, freq = topo.num_dofs, 3, 60, 20.0
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 3, "collisionMode": "convex", "worldCollisionMargin": 0.01,
              "analyticalGradientEpsilon": 1e-7, "ignoreLinksForCollision": [names[1], names[3], names[5]]}
    cs = collision_set(topo, {}, config, hulls=hulls, world_hulls=wh)
    nf = [2] * n

    def make(x):
        a = [x[1 + n + 2 * j:1 + n + 2 * j + 2] for j in range(n)]
        b = [x[1 + 3 * n + 2 * j:1 + 3 * n + 2 * j + 2] for j in range(n)]
        return exc.fourier_coefficients(a, b, x[1:1 + n], nf, wf=float(x[0]))

    xs = [np.concatenate([[rng.uniform(0.8, 1.2)], rng.uniform(-0.2, 0.2, n), rng.standard_normal(4 * n) * 0.5]) for _ in range(C)]
    return {"topo": topo, "cs": cs, "config": config, "nf": nf, "make": make, "xs": xs, "C": C, "T": Tn, "freq": freq}


def host_positions(cand, Tn, freq):
    """q (T, n) of one candidate from the series restatement (tests/fourier_gradient_restatement.py)"""
    import fourier_gradient_restatement as frest

    t = np.arange(Tn) / freq
    qr = cand["q_range"]
    return np.stack([frest.series(cand["wf"], cand["q_offset"][j], None if qr is None else qr[j], cand["a"][j], cand["b"][j], t)[0]
                     for j in range(len(cand["q_offset"]))], axis=1)


def variable_differences(block, x, margins):
    """Central differences of a candidate's collision block over +- E2E_STEP in every optimiser variable.  block(x) -> (g (P,), idx (P,)).
    Returns (fd (P, len(x)), keep (P,)): ``keep`` leaves out the pairs no configuration won, those whose winning configuration changes
    anywhere on the stencil, and those whose centre distance g + margin is <= 0."""
    g0, i0 = block(x)
    keep = (g0 < 1e10) & (g0 + margins > 0)
    fd = np.zeros((g0.size, x.size))
    for v in range(x.size):
        xp, xm = x.copy(), x.copy()
        xp[v] += E2E_STEP
        xm[v] -= E2E_STEP
        (gp, ip), (gm, im) = block(xp), block(xm)
        keep &= (ip == i0) & (im == i0)
        fd[:, v] = (gp - gm) / (2.0 * E2E_STEP)
    return fd, keep


def restated_rows(case, cons, q, cands, c, eps):
    """candidate c: the restated grad_q at the evaluation points of ``cons`` (in the reference's pair order) chained in long double,
    (ref of hull_gradient_restatement.evaluate with its bars, rows (P, E), the bound per row and parameter)"""
    import capsule_gradient_restatement as cg

    topo, cs = case["topo"], case["cs"]
    tup = as_tuples(topo, cs["hulls"])
    hp = np.asarray(cs["hull_pairs"]).reshape(-1, 2)[np.asarray(cs["columns"])[:, 1]]
    C = len(cands)
    mode = bool(cs.get("offset_in_link_axes", False))
    pick = lambda k: np.ascontiguousarray(np.asarray(cons[k]))  # noqa: E731
    ref = hg.evaluate(topo, tup, hp, False, q, None, None, C, pick("eval_sample"), pick("eval_scale"), pick("eval_pose"), eps, mode)
    sub = {"topo": topo, "floating": False, "hulls": cs["hulls"], "pairs": hp, "q": q, "rpy": None, "bp": None}
    ed, _ = emul_evaluate(sub, C, pick("eval_sample"), pick("eval_scale"), pick("eval_pose"), eps, mode, hp)
    fin = np.isfinite(ref["dist"]) & ~ref["none"]
    ref = hg.with_dev(ref, float(np.abs(ed - ref["dist"])[fin].max()))
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


def test_end_to_end_seed_with_the_restatement_alone():
    """The experiment of tests/test_gpu_hull_gradient.py's end-to-end test without the device: the collision block of one candidate from
    the Qhull restatement (test_hulls.HostHullEngine), differenced over +-1e-6 in every optimiser variable, against the restated central
    differences at eps = 1e-7 chained to the variables.  Gives the bar of the device's comparison (ten times the figure here) and checks that
    the committed seed leaves out at most a quarter of the rows.
    Measured: max |row - FD| = 4.2e-9 over 13 of the 14 rows (4 won by a transition configuration), max |row| 1.7: E2E_FD_BAR = 5e-8."""
    from flobaroid_amd import excitation as exc
    from test_hulls import HostHullEngine

    case = e2e_case()
    topo, cs, config, C, Tn, freq = case["topo"], case["cs"], case["config"], case["C"], case["T"], case["freq"]
    P, n = len(cs["pair_names"]), topo.num_dofs
    assert np.all(np.asarray(cs["columns"])[:, 0] == 2) and 6 <= P <= 16
    cands = [case["make"](x) for x in case["xs"]]
    q = np.concatenate([host_positions(cd, Tn, freq) for cd in cands])
    eng = HostHullEngine(topo, False)
    cons = exc._collision_block(eng, {"q": q}, C, config, cs)
    trans = (cons["idx"] < 0) & (cons["g"] < 1e10)
    c = int(np.argmax(trans.sum(axis=1)))
    assert trans[c].any(), "no transition configuration wins a pair: choose another seed"
    ref, want, _ = restated_rows(case, cons, q, cands, c, 1e-7)
    nh = cands[c]["a"].shape[1]
    rows = exc.constraint_gradient_to_optimizer_variables({k: v for k, v in exc._gradient_dict(want, n, nh).items()}, cands[c], case["nf"])
    margins = np.asarray(cs["margins"], dtype=np.float64)

    def block(x):
        b = exc._collision_block(eng, {"q": host_positions(case["make"](x), Tn, freq)}, 1, config, cs)
        return b["g"][0], b["idx"][0]

    fd, keep = variable_differences(block, case["xs"][c], margins)
    err = np.abs(fd - rows)[keep].max()
    print(f"restatement alone: candidate {c}, {int(keep.sum())} of {P} rows kept ({int(trans[c].sum())} won by a transition configuration), "
          f"max |row - FD| = {err:.2e}, max |row| = {np.abs(rows[keep]).max():.3f}")
    assert keep.sum() >= (1.0 - E2E_MAX_EXCLUDED) * P, "more than a quarter of the rows are left out: choose another seed"
    assert 10.0 * err <= E2E_FD_BAR and np.abs(rows[keep]).max() > 1e-2


# ---- excitation: the hull rows against a stub engine -----------------------------------------------------------------------------------------
class StubEngine:
    """marks what the hull gradient call returns: rows 3000 + 10 pair + joint; the chain is the identity padded to the chain's width"""
    floating, n = False, 3

    def __init__(self):
        self.calls = []

    def set_capsules(self, *a, **k):
        raise AssertionError("convex mode installs no capsules")

    set_boxes = set_capsules

    def set_hulls(self, hulls, pairs, offset_in_link_axes=False):
        self.nhull = len(pairs)
        self.calls.append(("set_hulls", offset_in_link_axes))

    def hull_distance_gradients(self, st, C, sample, scale=None, pose_sample=None, base_pos=None, epsilon=None):
        self.calls.append(("hull_gradients", epsilon))
        P = self.nhull
        assert sample.shape == scale.shape == pose_sample.shape == (C, P)
        # the evaluation points carry the set's own pair number in their value (see the test)
        assert np.array_equal(sample, np.tile(np.arange(P) + 300, (C, 1))) and np.array_equal(pose_sample, sample + 1) and np.array_equal(scale, sample * 0.5)
        return {"dist": np.zeros((C, P)), "grad_q": 3000.0 + 10.0 * np.arange(P)[None, :, None] + np.arange(self.n)[None, None, :] + np.zeros((C, 1, 1))}

    def fourier_position_chain(self, wf, A, B, sample, grad_q, freq, scale=None, q_range=None):
        C, P, n = grad_q.shape
        out = np.zeros((C, P, 1 + 2 * n + 2 * n * A.shape[2]))
        out[:, :, 1:1 + n] = grad_q
        return out


def test_hull_rows_against_a_stub_engine():
    from flobaroid_amd import excitation as exc

    C, n, nh = 2, 3, 2
    columns = np.array([[2, 2], [2, 0], [2, 3], [2, 1]])  # the reference's order: hull pairs 2, 0, 3, 1
    cs = {"capsules": [], "pairs": np.zeros((0, 2)), "hulls": ["h"] * 4, "hull_pairs": np.array([(0, 1), (0, 2), (1, 3), (2, 3)]), "columns": columns,
          "offset_in_link_axes": True}
    P = len(columns)
    own = columns[:, 1] + 300
    cons = {"g": np.arange(C * P, dtype=float).reshape(C, P), "eval_sample": np.tile(own, (C, 1)), "eval_scale": np.tile(own, (C, 1)) * 0.5,
            "eval_pose": np.tile(own, (C, 1)) + 1}
    cand = [{"wf": 1.0, "a": np.zeros((n, nh)), "b": np.zeros((n, nh)), "q_range": None}] * C
    st = {"q": np.zeros((C * 4, n))}
    convex = {"collisionMode": "convex", "analyticalGradientEpsilon": 3e-6}
    eng = StubEngine()
    out = exc.candidate_collision_gradient(eng, st, C, cand, 50.0, convex, cs, constraints=cons, hull_gradient=True)
    want = 3000.0 + 10.0 * columns[:, 1][None, :, None] + np.arange(n)[None, None, :] + np.zeros((C, 1, 1))
    assert np.array_equal(out["grad_q"], want) and np.array_equal(out["grad"]["q_offset"], want) and np.array_equal(out["g"], cons["g"])
    assert out["grad"]["a"].shape == (C, P, n, nh) and not out["grad"]["a"].any() and not out["grad"]["wf"].any()
    assert eng.calls == [("set_hulls", True), ("hull_gradients", 3e-6)]
    # the function's own epsilon wins over the configuration's; without either, the reference's default; box_gradient changes nothing
    for kw, eps in (({"epsilon": 1e-5}, 1e-5), ({"epsilon": 1e-5, "box_gradient": True}, 1e-5)):
        eng = StubEngine()
        exc.candidate_collision_gradient(eng, st, C, cand, 50.0, convex, cs, constraints=cons, hull_gradient=True, **kw)
        assert eng.calls == [("set_hulls", True), ("hull_gradients", eps)]
    eng = StubEngine()
    exc.candidate_collision_gradient(eng, st, C, cand, 50.0, {"collisionMode": "convex"}, dict(cs, offset_in_link_axes=False), constraints=cons,
                                     hull_gradient=True)
    assert eng.calls == [("set_hulls", False), ("hull_gradients", 1e-7)]
    # every refusal that must remain: without the keyword, in the other modes, the triangle-mesh mode, the suspended base
    for kw in ({}, {"hull_gradient": False}, {"box_gradient": True}):
        with pytest.raises(ValueError, match="no mesh code"):
            exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, convex, cs, constraints=cons, **kw)
        with pytest.raises(ValueError, match="hull pairs"):
            exc.candidate_gradients_from_coefficients(StubEngine(), cand, 4, 50.0, None, None, {}, [], convex, collision=cs, **kw)
    for mode in ("capsule", "box"):
        for kw in ({"hull_gradient": True}, {"hull_gradient": True, "box_gradient": True}):
            with pytest.raises(ValueError, match="hull pairs"):
                exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, {"collisionMode": mode}, cs, constraints=cons, **kw)
            with pytest.raises(ValueError, match="hull pairs"):
                exc.candidate_gradients_from_coefficients(StubEngine(), cand, 4, 50.0, None, None, {}, [], {"collisionMode": mode}, collision=cs, **kw)
    with pytest.raises(ValueError, match="no mesh code"):
        exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, {"collisionMode": "full"}, cs, constraints=cons, hull_gradient=True,
                                         box_gradient=True)
    with pytest.raises(ValueError, match="suspended"):
        exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, dict(convex, floatingBaseAttachment="suspended"), cs, constraints=cons,
                                         hull_gradient=True)
    # convex mode needs hull pairs, and only those
    with pytest.raises(ValueError, match="hull pairs"):
        exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, convex, {"capsules": ["c"] * 2, "pairs": [(0, 1)]}, constraints=cons,
                                         hull_gradient=True)
    with pytest.raises(ValueError, match="capsule or box pairs"):
        exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, convex, dict(cs, columns=np.array([[2, 0], [1, 0], [2, 1], [2, 2]])),
                                         constraints=cons, hull_gradient=True)


def test_hull_gradient_symbol_in_header_binding_and_library():
    """added under C-ABI 104: the version stays, header, binding and library carry the symbol"""
    from flobaroid_amd import _lib

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    name = "fbr_hull_distance_gradients"
    assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr)
    assert _lib._SIGNATURES[name] == _lib._SIGNATURES["fbr_box_distance_gradients"]
    assert lib.fbr_version() == _lib.FBR_VERSION == 104 == int(re.search(r"#define FBR_VERSION (\d+)", hdr).group(1))
    assert hasattr(_lib.Engine, "hull_distance_gradients")
    assert hr.EPS == hg.EPS
