"""The gradient of hulls above 128 vertices off the GPU (csrc/fbr_hull_large_grad.h, fbr_large_hull_distance_gradients).  Needs no GPU.

* (a) the three stages of the device on the host (tests/emul/hull_large_grad_emul.cpp route 1: recorded poses, one distance per pose with
  the wave's facet pass, the quotients) against the single pass (route 0: fbr_rigidgrad_item with fbr_hull_large_distance as its functor):
  the bytes of dist and grad, on the four robots of tests/test_box_gradient.py with two large hulls among the small ones, both offset
  modes, both steps, scale / pose_sample / sample = -1 entries.  On the sets of small hulls only, every pair through the stages (option
  hull_large_all) == tests/emul/hull_grad_emul.cpp (==, not bytes: the order of a maximum may change the sign of a zero gap).
* (b) known slopes on the large gantry of tests/test_gpu_hulls_large.py: a 257-point sphere on a 200-gon's cap, the 511-gon cone's apex
  on a 65-gon's cap, KUKA's wrist over its base, at the gaps 1e-9, 0, -1e-9, -1e-3: lift +-1, slide 0 within (b+ + b-) / (2 eps),
  b+- = 32 EPS x scale.  Whether a contact is one-sided at gap 0 is decided by the Qhull restatement's two one-sided slopes.
* (c) the emulation against the NumPy / Qhull restatement (tests/hull_gradient_restatement.py) on pairs Qhull restates in milliseconds.
* (d) excitation's large_hull_gradient keyword against a stub engine; (e) the symbol in header, binding and library.

Measured here (g++ 13, x86-64): (a) the bytes equal in all 16 cases (5 to 8 large pairs of 10 to 16, 85 to 420 stencil entries a call,
0.000 to 0.762 of them in the facet pass); (b) |row - expected| / bar 0.004 on the sphere and the cone, 0.015 on KUKA's wrist at eps =
1e-7 (0.001 / 0.003 at 1e-4), the same at every gap; by the restatement no contact is one-sided at gap 0 (slopes 1.000000001 above and
below); (c) largest |emulation - restatement| / bar: threeLinks 0.005, kuka_lwr4 0.021, lwr_base_link against lwr_7_link on KUKA 0.017.

Mutations (f), each made in a scratch copy of the tree and not committed:
* the + eps and - eps slots swapped in fbr_meshgrad_quotients (csrc/fbr_mesh_grad.h): all 16 cases of (a), (b) and the three tests of (c)
  fail -- 20 of 20;
* the facet join of fbr_hull_facets_wave taking >= (csrc/fbr_hull_large.h): no test fails, here or on the device, and none can by value --
  the join is a maximum, >= takes the later of two equal values, and only the sign of a zero gap can differ; the tests that compare the
  shared pass with the one-lane pass use == for that reason;
* the tile tail not excluded from the ballot (the device's stage B only; the host has no lanes): the repeated lanes would run facet
  passes of the last entry again and drop the results -- no value changes and no test fails; it costs time in stage B alone."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hull_gradient_restatement as hg
import hull_large_shapes as ls
import hull_restatement as hr
from common import ROOT
from test_box_gradient import ROBOTS, item_arrays
from test_hull_gradient import STACK_ROWS, case_of, emul_evaluate, make_case
from test_hulls import _c, _p, as_tuples, link_index, tables

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "hull_large_grad_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libhull_large_grad_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_lib = None
EPS = hg.EPS


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC, os.path.join(ROOT, "include", "fbr.h")] + [os.path.join(_CSRC, h) for h in (
            "fbr_hull_large_grad.h", "fbr_hull_large.h", "fbr_mesh_grad.h", "fbr_mesh.h", "fbr_hull_grad.h", "fbr_hull.h", "fbr_box_grad.h", "fbr_box.h",
            "fbr_capsule_grad.h", "fbr_capsule.h", "fbr_math.h", "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


def large_items(topo, floating, hulls, item_pairs, q, rpy, base_pos, mode, eps, route, every=False):
    """(dist (M,), grad (M, n), stencil points (M,), entries in the facet pass) of one hull pair per configuration; route 0: the single
    pass, 1: the three stages; ``every``: option hull_large_all"""
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
    dist, grad, ns, facet = np.zeros(M), np.full((M, topo.num_dofs), np.nan), np.zeros(M, dtype=np.int32), ctypes.c_long(0)
    rc = emul().hulllgrad_eval(topo.num_links, topo.num_dofs, _p(parent), _p(dof), _p(rR), _p(rp), _p(ax), _p(jt), int(floating), len(hulls), _p(link),
                               _p(off), _p(rot), int(mode), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), ctypes.c_double(eps), ctypes.c_long(M),
                               _p(pr), _p(q), _p(rpy), _p(bp), int(route), int(every), _p(dist), _p(grad), _p(ns), ctypes.byref(facet))
    assert rc == 0, rc
    return dist, grad, ns, int(facet.value)


def large_evaluate(case, C, sample, scale, pose, eps, mode, route, every=False, pairs=None, hulls=None):
    """the contract of fbr_large_hull_distance_gradients from the emulation: (dist (C, P), grad (C, P, n), stencil points (C, P), facet entries)"""
    topo, fl = case["topo"], case["floating"]
    pairs = case["pairs"] if pairs is None else pairs
    P, Tn = len(pairs), case["q"].shape[0] // C
    sample = np.asarray(sample).reshape(C, P)
    ps = sample if pose is None else np.where(np.asarray(pose) < 0, sample, pose)
    sc = np.ones((C, P)) if scale is None else np.asarray(scale)
    base = (np.arange(C) * Tn)[:, None]
    rq, rp = (base + np.maximum(sample, 0)).reshape(-1), (base + np.maximum(ps, 0)).reshape(-1)
    dist, grad, ns, facet = large_items(topo, fl, case["hulls"] if hulls is None else hulls, np.tile(pairs, (C, 1)), case["q"][rq] * sc.reshape(-1, 1),
                                        case["rpy"][rp] if fl else None, case["bp"][rp] if fl else None, mode, eps, route, every)
    none = sample < 0
    return np.where(none, hg.NONE, dist.reshape(C, P)), np.where(none[..., None], 0.0, grad.reshape(C, P, -1)), ns.reshape(C, P), facet


# ---- the cases (shared with tests/test_gpu_hull_large_gradient.py) ----------------------------------------------------------------------------
LARGE_ON = ("prism130", "lwr_7_link")  # the large shapes put on two robot links of every case, scaled to the size of the hull they replace


def with_large_hulls(case):
    """``case`` (tests/test_hull_gradient.py make_case) with the hulls of the first two robot links that sit in at least two pairs replaced
    by LARGE_ON, scaled to the replaced hull's diameter: (hulls, large (P,) bool)"""
    from flobaroid_amd.collision import Hull

    hulls = list(case["hulls"])
    count = np.bincount(case["pairs"].reshape(-1), minlength=len(hulls))
    robot = [i for i, h in enumerate(hulls) if h.link_name is not None and count[i] >= 2][:2]
    assert len(robot) == 2
    K = ls.kuka_hulls()
    for i, kind in zip(robot, LARGE_ON):
        src = K[kind] if kind in K else ls.shape(kind)
        pts = src.vertices - src.vertices.mean(axis=0)
        hulls[i] = Hull(hulls[i].link_name, pts * (hulls[i].diameter / src.diameter), hulls[i].offset)
        assert len(hulls[i].vertices) == len(src.vertices) > 128
    big = np.array([len(h.vertices) > 128 for h in hulls])
    return hulls, big[case["pairs"]].any(axis=1)


# ---- (a) the stages equal the single pass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-7, 1e-4])
@pytest.mark.parametrize("mode", [False, True], ids=["world-axes", "link-axes"])
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_three_stages_equal_the_single_pass_bit_for_bit(robot, mode, eps):
    case = case_of(robot)
    C, P = case["C"], len(case["pairs"])
    hulls, large = with_large_hulls(case)
    assert 2 <= large.sum() < P
    rng = np.random.default_rng(12)
    for with_scale in (False, True):
        sample, scale, pose = item_arrays(case, rng, C, P, with_scale)
        assert (sample < 0).any() and (sample >= 0).any()
        d0, g0, n0, _ = large_evaluate(case, C, sample, scale, pose, eps, mode, 0, hulls=hulls)
        d1, g1, n1, facet = large_evaluate(case, C, sample, scale, pose, eps, mode, 1, hulls=hulls)
        live = sample >= 0
        assert d0.tobytes() == d1.tobytes() and g0.tobytes() == g1.tobytes()
        # the stencil of a large pair: the centre and two points a joint with an entry; a small pair records nothing
        assert np.all(n1[:, ~large] == 0) and np.all(n1[:, large] >= 1) and np.all(n1[:, large] % 2 == 1) and n1.max() >= 3
        ent = int(n1.sum())
        print(f"{robot} mode {int(mode)} eps {eps:g} scale {with_scale}: {int(large.sum())} large pairs of {P}, {ent} stencil entries, "
              f"{facet / ent:.3f} of them in the facet pass; centre distances <= 0: {(d1[live] <= 0).mean():.2f}")
        assert np.isfinite(g1).all() and np.abs(g1[:, large]).max() > 1e-2
        # every pair through the stages on the set of small hulls: the values of the one-lane routine
        de, ge = emul_evaluate(case, C, sample, scale, pose, eps, mode)
        da, ga, na, _ = large_evaluate(case, C, sample, scale, pose, eps, mode, 1, every=True)
        assert np.array_equal(da, de) and np.array_equal(ga, ge) and np.all(na >= 1)
        dz, gz, nz, _ = large_evaluate(case, C, sample, scale, pose, eps, mode, 1, every=False)
        assert dz.tobytes() == de.tobytes() and gz.tobytes() == ge.tobytes() and not nz.any()


def test_tile_width_rule():
    """fbr_hull_large_grad_width: the widest power of two that leaves `want` items, 1 where the entries do not allow it"""
    sbeg = _c(np.cumsum([0, 15, 13, 11, 9, 7, 5, 3]), np.int32)  # KUKA's floor pairs: 1 + 2 J points
    w = lambda C, want: emul().hulllgrad_width(_p(sbeg), 7, ctypes.c_long(C), ctypes.c_long(want))  # noqa: E731
    # 63 points: 63 C entries; C = 64: 4032 entries are 2016 items of 2 and 1008 of 4; C = 1: 11 items of 8, 7 of 16 and wider
    assert w(1, 1024) == 1 and w(2, 1024) == 1 and w(64, 1024) == 2 and w(4096, 1024) == 64 and w(1, 8) == 8 and w(1, 7) == 64 and w(1, 1) == 64


# ---- (b) known slopes on the large gantry ---------------------------------------------------------------------------------------------------
CONTACTS = {"sphere257 on the 200-gon's cap": (400, 257), "cone512's apex on the 65-gon's cap": (130, 512), "KUKA's wrist over its base": (216, 793)}


def contact_columns():
    """(topo, hulls, pairs, q, {name: pair index}) of tests/test_gpu_hulls_large.py large_gantry_case: the three contact columns"""
    from test_gpu_hulls_large import large_gantry_case

    topo, hl, pairs, q = large_gantry_case()[:4]
    nv = np.array([len(h.vertices) for h in hl])
    cols = {}
    for name, (va, vb) in CONTACTS.items():
        k = [i for i, (a, b) in enumerate(pairs) if nv[a] == va and nv[b] == vb and hl[a].link_name == "bed" and hl[b].link_name == "carriage"]
        assert len(k) == 1, name
        cols[name] = k[0]
    return topo, hl, pairs, q, cols


def test_known_slopes_on_the_large_gantry():
    from test_gpu_hulls import GAPS, TOUCH, TT

    topo, hl, pairs, q, cols = contact_columns()
    tup = as_tuples(topo, hl)
    diam = hg.diameters(tup)
    sel = np.array(list(cols.values()))
    for eps in (1e-7, 1e-4):
        for c, (gap, k0) in enumerate(zip(GAPS, TOUCH)):
            qc = np.repeat(q[c * TT + k0][None], len(sel), axis=0)
            for route in (0, 1):
                d, g, ns, _ = large_items(topo, False, hl, pairs[sel], qc, None, None, True, eps, route)
                assert np.all(ns == (0 if route == 0 else 5))
                if route == 0:
                    d0, g0 = d, g
            assert d.tobytes() == d0.tobytes() and g.tobytes() == g0.tobytes()
            R, cen = hr.hull_world(topo, tup, qc[:1], False, None, None, True)
            for j, (name, k) in enumerate(cols.items()):
                a, b = pairs[k]
                scale = float(hr.pair_scale(cen[0, a], diam[a], cen[0, b], diam[b]))
                bar = 2.0 * (32.0 * EPS * scale) / (2.0 * eps)
                one_sided = False
                if gap == 0.0:
                    # the restatement's two one-sided slopes in the lift: a contact feature whose depth does not continue the distance
                    dd = []
                    for s in (1.0, 0.0, -1.0):
                        qq = qc[:1] + np.array([[s * eps, 0.0]])
                        Rw, cw = hr.hull_world(topo, tup, qq, False, None, None, True)
                        dd.append(hr.hull_distance(Rw[0, a], cw[0, a], hl[a].vertices, Rw[0, b], cw[0, b], hl[b].vertices))
                    up, down = (dd[0] - dd[1]) / eps, (dd[1] - dd[2]) / eps
                    one_sided = abs(up - down) > 2.0 * bar
                    print(f"{name}, gap 0, eps {eps:g}: the restatement's slopes in the lift {up:.9f} above, {down:.9f} below"
                          + (" -- one-sided, the row is not asserted here (the gaps +-1e-9 are)" if one_sided else ""))
                err = np.abs(g[j] - STACK_ROWS[0])
                print(f"{name}, gap {gap:g}, eps {eps:g}: dist {d[j]:.3e}, row {g[j]}, |row - expected| / bar = {(err / bar).max():.3f} (bar {bar:.2e})")
                assert abs(d[j] - gap) <= 32.0 * EPS * scale
                if not one_sided:
                    assert np.all(err <= bar), (name, gap, eps)


# ---- (c) the emulation against the restatement ------------------------------------------------------------------------------------------------
def restated_case(robot):
    """a world box, a small hull and a large one on the robot: the pairs Qhull restates in milliseconds -- (case, hulls, pairs)"""
    case = make_case(robot, C=3)
    hulls, large = with_large_hulls(case)
    nv = np.array([len(h.vertices) for h in hulls])
    ok = np.array([min(nv[a], nv[b]) <= 12 for a, b in case["pairs"]]) & large
    assert ok.sum() >= 2
    return case, hulls, np.ascontiguousarray(case["pairs"][ok][:4])


@pytest.mark.parametrize("robot", ["threeLinks", "kuka_lwr4"])
def test_emulation_equals_the_restatement_on_large_pairs(robot):
    """the project's rule of tests/test_gpu_hull_gradient.py: (b+ + b-) / (2 eps), b+- = max(10 dev, 32 EPS scale), dev the emulation's
    largest deviation from the restatement over the case's centre distances"""
    case, hulls, pairs = restated_case(robot)
    C, P = 3, len(pairs)
    rng = np.random.default_rng(13)
    tup = as_tuples(case["topo"], hulls)
    for mode in (False, True):
        sample, scale, pose = item_arrays(case, rng, C, P, True)
        ref = hg.evaluate(case["topo"], tup, pairs, case["floating"], case["q"], case["rpy"], case["bp"], C, sample, scale, pose, 1e-7, mode)
        ed, eg, ns, _ = large_evaluate(case, C, sample, scale, pose, 1e-7, mode, 1, pairs=pairs, hulls=hulls)
        live = ~ref["none"]
        ref = hg.with_dev(ref, float(np.abs(ed - ref["dist"])[live].max()))
        worst = (np.abs(eg - ref["grad"]) / ref["bar"]).max()
        print(f"{robot} mode {int(mode)}: {P} large pairs, max |delta grad| / bar = {worst:.3f}, max |grad| = {np.abs(ref['grad']).max():.3f}, "
              f"centre distances <= 0: {(ref['dist'][live] <= 0).sum()} of {live.sum()}")
        assert np.all(np.abs(ed - ref["dist"])[live] <= ref["dist_bar"][live]) and np.all(ed[~live] == hg.NONE)
        assert np.all(np.abs(eg - ref["grad"]) <= ref["bar"])
        assert np.all(eg[~ref["on_path"]] == 0.0) and np.all(eg[~live] == 0.0) and np.abs(ref["grad"]).max() > 1e-2


def test_emulation_equals_the_restatement_on_kuka_base_against_wrist():
    """lwr_base_link against lwr_7_link on KUKA itself, both above 128 vertices"""
    from common import load_topo

    topo = load_topo("kuka_lwr4")
    K = ls.kuka_hulls()
    hulls = [K["lwr_base_link"], K["lwr_7_link"]]
    pairs = np.array([[0, 1], [1, 0]], dtype=np.int32)
    rng = np.random.default_rng(14)
    C, Tn = 2, 2
    # bent back so that the flange comes near the base
    q = np.array([0.3, 1.9, -0.4, -2.0, 0.5, 1.9, 0.2]) + rng.uniform(-0.05, 0.05, (C * Tn, 7))
    case = {"topo": topo, "floating": False, "hulls": hulls, "pairs": pairs, "q": q, "rpy": None, "bp": None}
    sample = np.array([[0, 1], [1, 0]])
    tup = as_tuples(topo, hulls)
    ref = hg.evaluate(topo, tup, pairs, False, q, None, None, C, sample, None, None, 1e-7, False)
    ed, eg, ns, _ = large_evaluate(case, C, sample, None, None, 1e-7, False, 1)
    ref = hg.with_dev(ref, float(np.abs(ed - ref["dist"]).max()))
    worst = (np.abs(eg - ref["grad"]) / ref["bar"]).max()
    print(f"KUKA base against wrist: dist {ed.reshape(-1)}, max |delta grad| / bar = {worst:.3f}, max |grad| = {np.abs(ref['grad']).max():.3f}")
    assert np.all(ns == 15) and np.all(np.abs(ed - ref["dist"]) <= ref["dist_bar"]) and np.all(np.abs(eg - ref["grad"]) <= ref["bar"])
    assert np.abs(ref["grad"]).max() > 1e-2


# ---- KUKA end to end (shared with tests/test_gpu_hull_large_gradient.py) ----------------------------------------------------------------------
def kuka_case(engine_states):
    """The setting of tests/test_gpu_hulls_large.py test_kuka_convex_collision_block_and_the_gradient_refusal: fixed base, the eight hulls of
    the fixture over the floor of world_kuka.urdf, 7 pairs (the floor against lwr_2_link .. lwr_7_link, lwr_base_link against lwr_7_link),
    C = 2, T = 64, collisionCheckStep 1, transitions on.  ``engine_states(cands, T, freq)`` -> q (C T, n) on the host."""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd.collision import collision_set, world_hulls_from_urdf
    from common import GOLDEN, load_topo

    topo = load_topo("kuka_lwr4")
    K = ls.kuka_hulls()
    rng = np.random.default_rng(35)
    n, C, Tn, freq = topo.num_dofs, 2, 64, 100.0
    arm = [f"lwr_{i}_link" for i in range(1, 8)]
    config = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0, "collisionCheckStep": 1,
              "transitionDuration": 3.0, "transitionCollisionSamples": 1, "collisionMode": "convex", "worldCollisionMargin": 0.01,
              "analyticalGradientEpsilon": 1e-7,
              "ignoreLinkPairsForCollision": [[a, b] for i, a in enumerate(arm) for b in arm[i + 1:]] + [["lwr_base_link", a] for a in arm[:6]]
              + [["ground_link", "lwr_base_link"], ["ground_link", "lwr_1_link"]]}
    posture = np.array([0.3, 1.9, -0.4, -1.2, 0.5, 0.9, 0.2])
    cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.02 for _ in range(n)], [rng.standard_normal(2) * 0.02 for _ in range(n)],
                                      posture + rng.uniform(-0.02, 0.02, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    q = engine_states(cands, Tn, freq)
    wh = world_hulls_from_urdf(os.path.join(GOLDEN, "urdf", "world_kuka.urdf"), "geometric")
    tup7 = as_tuples(topo, [K["lwr_7_link"]])
    R7, c7 = hr.hull_world(topo, tup7, q[:1], False, None, None, False)
    low = float((c7[0, 0] + K["lwr_7_link"].vertices @ R7[0, 0].T)[:, 2].min())
    wh["ground_link"].offset = wh["ground_link"].offset + np.array([0.0, 0.0, low - 0.012])  # its top 2 mm inside the margin below the flange
    cs = collision_set(topo, {}, config, hulls=K, world_hulls=wh)
    return {"topo": topo, "cs": cs, "config": config, "cands": cands, "q": q, "C": C, "T": Tn, "freq": freq}


def restated_rows_large(case, cons, q, cands, c, eps):
    """tests/test_hull_gradient.py restated_rows with this file's emulation for the deviation of the centre distances (that file's refuses
    hulls above 128 vertices): (ref with its bars, rows (P, E) of candidate c chained in long double, the bound per row and parameter)"""
    import capsule_gradient_restatement as cg

    topo, cs = case["topo"], case["cs"]
    tup = as_tuples(topo, cs["hulls"])
    hp = np.asarray(cs["hull_pairs"]).reshape(-1, 2)[np.asarray(cs["columns"])[:, 1]]
    C = len(cands)
    mode = bool(cs.get("offset_in_link_axes", False))
    pick = lambda k: np.ascontiguousarray(np.asarray(cons[k]))  # noqa: E731
    ref = hg.evaluate(topo, tup, hp, False, q, None, None, C, pick("eval_sample"), pick("eval_scale"), pick("eval_pose"), eps, mode)
    sub = {"topo": topo, "floating": False, "hulls": cs["hulls"], "pairs": hp, "q": q, "rpy": None, "bp": None}
    ed, eg, _, facet = large_evaluate(sub, C, pick("eval_sample"), pick("eval_scale"), pick("eval_pose"), eps, mode, 1)
    fin = np.isfinite(ref["dist"]) & ~ref["none"]
    ref = dict(hg.with_dev(ref, float(np.abs(ed - ref["dist"])[fin].max())), emul_dist=ed, emul_grad=eg, facet=facet)
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


# ---- (d) excitation: the keyword against a stub engine ------------------------------------------------------------------------------------------
class _Hull:
    def __init__(self, name, nv):
        self.link_name, self.name, self.vertices = name, name, np.zeros((nv, 3))


class StubEngine:
    """marks what the large-hull gradient call returns: rows 7000 + 10 pair + joint; the chain is the identity padded to the chain's width"""
    floating, n = False, 3

    def __init__(self):
        self.calls = []

    def set_capsules(self, *a, **k):
        raise AssertionError("convex mode installs no capsules")

    set_boxes = set_capsules

    def set_hulls(self, hulls, pairs, offset_in_link_axes=False, **kw):
        self.nhull = len(pairs)
        self.calls.append(("set_hulls", offset_in_link_axes, kw))

    def hull_distance_gradients(self, *a, **k):
        raise AssertionError("a large set goes to large_hull_distance_gradients")

    mesh_distance_gradients = hull_distance_gradients

    def large_hull_distance_gradients(self, st, C, sample, scale=None, pose_sample=None, base_pos=None, epsilon=None):
        self.calls.append(("large_hull_gradients", epsilon))
        P = self.nhull
        assert sample.shape == scale.shape == pose_sample.shape == (C, P)
        assert np.array_equal(sample, np.tile(np.arange(P) + 300, (C, 1))) and np.array_equal(pose_sample, sample + 1) and np.array_equal(scale, sample * 0.5)
        return {"dist": np.zeros((C, P)), "grad_q": 7000.0 + 10.0 * np.arange(P)[None, :, None] + np.arange(self.n)[None, None, :] + np.zeros((C, 1, 1))}

    def fourier_position_chain(self, wf, A, B, sample, grad_q, freq, scale=None, q_range=None):
        C, P, n = grad_q.shape
        out = np.zeros((C, P, 1 + 2 * n + 2 * n * A.shape[2]))
        out[:, :, 1:1 + n] = grad_q
        return out


def test_large_hull_rows_against_a_stub_engine():
    from flobaroid_amd import excitation as exc

    C, n, nh = 2, 3, 2
    columns = np.array([[2, 2], [2, 0], [2, 3], [2, 1]])  # the reference's order: hull pairs 2, 0, 3, 1
    hulls = [_Hull("base", 8), _Hull("lwr_6_link", 793), _Hull("lwr_7_link", 158), _Hull("tool", 12)]
    cs = {"capsules": [], "pairs": np.zeros((0, 2)), "hulls": hulls, "hull_pairs": np.array([(0, 1), (0, 2), (1, 3), (2, 3)]), "columns": columns,
          "offset_in_link_axes": True}
    P = len(columns)
    own = columns[:, 1] + 300
    cons = {"g": np.arange(C * P, dtype=float).reshape(C, P), "eval_sample": np.tile(own, (C, 1)), "eval_scale": np.tile(own, (C, 1)) * 0.5,
            "eval_pose": np.tile(own, (C, 1)) + 1}
    cand = [{"wf": 1.0, "a": np.zeros((n, nh)), "b": np.zeros((n, nh)), "q_range": None}] * C
    st = {"q": np.zeros((C * 4, n))}
    convex = {"collisionMode": "convex", "analyticalGradientEpsilon": 3e-6}
    want = 7000.0 + 10.0 * columns[:, 1][None, :, None] + np.arange(n)[None, None, :] + np.zeros((C, 1, 1))
    # the keyword routes the set, installed with large=True, to the new call; hull_gradient may be either value; the merge into pair order
    for kw, eps in (({}, 3e-6), ({"hull_gradient": True}, 3e-6), ({"hull_gradient": False, "epsilon": 1e-5}, 1e-5), ({"box_gradient": True}, 3e-6)):
        eng = StubEngine()
        out = exc.candidate_collision_gradient(eng, st, C, cand, 50.0, convex, cs, constraints=cons, large_hull_gradient=True, **kw)
        assert np.array_equal(out["grad_q"], want) and np.array_equal(out["grad"]["q_offset"], want) and np.array_equal(out["g"], cons["g"])
        assert out["grad"]["a"].shape == (C, P, n, nh) and not out["grad"]["a"].any() and not out["grad"]["wf"].any()
        assert eng.calls == [("set_hulls", True, {"large": True}), ("large_hull_gradients", eps)]
    # without the keyword: the refusal of before, word for word, whatever the other keywords say
    text = ("gradients on the device do not cover hulls of more than 128 vertices: the collision set has lwr_6_link (793 vertices), lwr_7_link (158 vertices)"
            "; the constraint values are served (Engine.set_hulls(..., large=True)), their gradients are not built")
    for kw in ({}, {"hull_gradient": True}, {"mesh_gradient": True}, {"box_gradient": True}, {"large_hull_gradient": False}):
        with pytest.raises(ValueError) as e:
            exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, convex, cs, constraints=cons, **kw)
        assert str(e.value) == text
        with pytest.raises(ValueError) as e:
            exc.candidate_gradients_from_coefficients(StubEngine(), cand, 4, 50.0, None, None, {}, [], convex, collision=cs, **kw)
        assert str(e.value) == text
    # every new ValueError says which condition fails
    small = dict(cs, hulls=[_Hull(h.name, min(len(h.vertices), 128)) for h in hulls])
    meshed = dict(cs, meshes={0: np.zeros((1, 3, 3))})
    mixed = dict(cs, columns=np.array([[2, 0], [1, 0], [2, 1], [2, 2]]))
    for config, cset, msg in (({"collisionMode": "capsule"}, cs, "collisionMode 'capsule' is not 'convex'"), ({"collisionMode": "box"}, cs, "is not 'convex'"),
                              ({"collisionMode": "full"}, cs, "is not 'convex'"), (convex, small, "no hull above 128 vertices"),
                              (convex, meshed, "triangle meshes"), (dict(convex, fullMeshLinks=["base"]), cs, "fullMeshLinks"),
                              (convex, mixed, "capsule or box pairs"), (convex, {"capsules": ["c"] * 2, "pairs": [(0, 1)]}, "needs a collision set with hull pairs")):
        with pytest.raises(ValueError, match="large_hull_gradient=True: .*" + msg):
            exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, config, cset, constraints=cons, large_hull_gradient=True)
        with pytest.raises(ValueError, match="large_hull_gradient=True: .*" + msg):
            exc.candidate_gradients_from_coefficients(StubEngine(), cand, 4, 50.0, None, None, {}, [], config, collision=cset, large_hull_gradient=True)
    # the suspended base stays refused in the gradient path
    with pytest.raises(ValueError, match="suspended"):
        exc.candidate_collision_gradient(StubEngine(), st, C, cand, 50.0, dict(convex, floatingBaseAttachment="suspended"), cs, constraints=cons,
                                         large_hull_gradient=True)
    import inspect

    for f in (exc.candidate_collision_gradient, exc.candidate_collision_gradient_from_coefficients, exc.candidate_gradients_from_coefficients):
        assert inspect.signature(f).parameters["large_hull_gradient"].default is False


# ---- (e) the symbol -----------------------------------------------------------------------------------------------------------------------------
def test_large_hull_gradient_symbol_in_header_binding_and_library():
    """added under C-ABI 104: the version stays, header, binding and library carry the symbol and the option"""
    from flobaroid_amd import _lib

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    name = "fbr_large_hull_distance_gradients"
    assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr)
    assert _lib._SIGNATURES[name] == _lib._SIGNATURES["fbr_hull_distance_gradients"]
    assert lib.fbr_version() == _lib.FBR_VERSION == 104 == int(re.search(r"#define FBR_VERSION (\d+)", hdr).group(1))
    assert hasattr(_lib.Engine, "large_hull_distance_gradients")
    assert '"hull_grad_tile"' in hdr and "hull_grad_tile" in open(os.path.join(_CSRC, "fbr_options.h")).read()
    names, i, p = [], 0, ctypes.c_char_p()
    while lib.fbr_model_option_name(i, ctypes.byref(p)) == 0:
        names.append(p.value.decode())
        i += 1
    assert "hull_grad_tile" in names and "hull_large_all" in names
    assert "fbr_hull_large_grad.h" in open(os.path.join(_CSRC, "fbr_collision_api.hip")).read()
