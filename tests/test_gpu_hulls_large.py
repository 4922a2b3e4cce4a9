"""Hulls of 129 to 1024 vertices on the device: Engine.set_hulls(..., large=True) / fbr_model_set_large_hulls and
fbr_hull_large_pairs_kernel (csrc/fbr_hull_large.h), in which the 64 lanes of a wave share the facet pass of a touching sample.

* Same device, two kernels: the small hulls and shuffled pairs of the exact contacts on the gantry (tests/test_gpu_hulls.py gantry_case)
  through set_hulls, and through set_hulls(large=True) with option hull_large_all = 1, which sends every pair to the new kernel: dist equal
  (np.array_equal: the sign of a zero gap may depend on the order in which a maximum is taken), idx identical.  C = 4 and 2, T = 67,
  step 1, host and device states; the contacts at 1e-9, 0, -1e-9 and -1e-3 are each reached in one lane; a candidate in which every
  sample of the four contact pairs overlaps fills a block with touching lanes.
* Large shapes on the gantry (tests/hull_large_shapes.py): the device against the emulation (frames from the library's lane walk through
  tests/emul/hull_emul.cpp, distances from tests/emul/hull_large_emul.cpp) within 32 eps x scale at the winning sample -- the smaller of
  the two terms of the project's bar, so no restatement is needed here; tests/test_hulls_large.py holds the emulation to the same figure
  against Qhull --, every index the emulation's argmin wherever the runner-up lies more than 100 bars above the minimum (at most 5 % of
  the columns may be excluded, asserted before the device is called); the same bits with chunk_samples 64, with each candidate alone
  and on a second run.
* Mixed set: the columns of the pairs of two small hulls are bytes-equal to the same pairs through fbr_model_set_hulls.
* KUKA LWR4 with the eight hulls of its visual meshes over the floor of world_kuka.urdf: the collision block of
  candidate_objectives_from_coefficients in collisionMode "convex" against the sample-by-sample restatement of the block (Qhull), and the
  gradient entry point's refusal by link and count.
* Refusals: 1025 vertices, set_hulls (not large) with 130, meshes on a large set, both gradient calls; the set in place returns its bytes.

Seen on an MI355X ("Large convex hulls"): the two kernels equal on all 18 pairs in every configuration; on the large gantry
the device returns the emulation's bits in all 68 columns (bars from 3.5e-15; 6.8 % of the evaluations in the facet pass, 16 GJK iterations
at most, no column excluded for a near tie); KUKA's block within 1.2e-16 = 0.022 bars of the restatement (bars from 5.0e-15)."""
import functools
import os

import numpy as np
import pytest

import hull_large_shapes as ls
import hull_restatement as hr
import hull_shapes as hs
from common import GOLDEN, load_topo
from test_gpu_boxes import _dev, _engine, _host
from test_gpu_hulls import GAPS, LIFT, TOUCH, TT, gantry_case
from test_hulls import EPS, as_tuples, emul_distance, emul_eval
from test_hulls_large import large_distance

pytestmark = pytest.mark.gpu
BATCH = 4  # FBR_HULL_LARGE_BATCH
SMALL = 128  # FBR_MAX_HULL_VERTICES


def _call(eng, q, ncand, device=True):
    return _host(eng.candidate_hull_distances(_dev({"q": q}) if device else {"q": q}, ncand, 1))


def _same(a, b):
    return a["dist"].tobytes() == b["dist"].tobytes() and a["idx"].tobytes() == b["idx"].tobytes()


# ---- the same pairs through the two kernels ---------------------------------------------------------------------------------------------------
def test_small_hulls_through_both_kernels_return_equal_distances():
    topo, hl, pairs, st, ref, contact = gantry_case("apex_down", True)
    assert max(len(h.vertices) for h in hl) == SMALL and len(pairs) > BATCH and len(pairs) % BATCH != 0
    q4 = st["q"]  # four candidates, one gap each, reached in one lane
    # two candidates: every sample of the first overlaps in the four contact pairs (1 to 3 mm deep), the second is the 1e-9 one
    i = np.arange(TT)
    deep = np.stack([(LIFT - 2.0 ** -10) - i * 2.0 ** -15, np.zeros(TT)], axis=1)  # (no slide: an apex stays on its apex)
    q2 = np.concatenate([deep, q4[:TT]])
    assert (emul_eval(topo, False, hl, pairs[contact], deep, None, None, True)[2] >= 1000).all()  # every sample enters the facet pass there
    small, large = _engine(topo, False), _engine(topo, False, options={"hull_large_all": 1})
    small.set_hulls(hl, pairs, offset_in_link_axes=True)
    large.set_hulls(hl, pairs, offset_in_link_axes=True, large=True)
    for q, C in ((q4, 4), (q2, 2)):
        for device in (False, True):
            a, b = _call(small, q, C, device), _call(large, q, C, device)
            assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["dist"], b["dist"]), (C, device)
            assert (a["dist"] <= 0).any() and (a["dist"] > 0).any()
    assert np.all(a["dist"][0, contact] < -0.25e-3) and np.all(a["dist"][0, contact] > -3.1e-3)  # the block in which every lane touches
    got4 = _call(small, q4, 4)
    assert np.array_equal(got4["idx"][:, contact], np.array(TOUCH)[:, None].repeat(len(contact), axis=1))  # each gap reached in its lane
    # the option is read by every call: switched off, the large set is split by size -- all pairs are small -- and returns the small kernel's bytes
    large.set_option("hull_large_all", 0)
    assert _same(_call(large, q4, 4), got4)
    large.set_option("hull_large_all", 1)
    assert np.array_equal(_call(large, q4, 4)["dist"], got4["dist"])
    # without the large entry point the option changes nothing
    small.set_option("hull_large_all", 1)
    assert _same(_call(small, q4, 4), got4)
    small.close()
    large.close()


# ---- large shapes on the gantry ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large_gantry_case():
    """Six columns, 1.5 m apart in x, of a hull on the bed and a hull on the carriage (turned by pi about x) that touch near the lift 0.25:
    a 257-point sphere's vertex on a 200-gon's cap, a 256-point sphere on a 1024-point one, the apex of the 511-gon cone on a 65-gon's cap,
    KUKA's wrist (793 vertices) over its base (216); two columns of small hulls, a cone's apex on a cube and a roof's edge on a ridge.
    The pairs: the six contacts, cross pairs, a tilted world box with every carriage hull, first or second; shuffled: 11 pairs with a hull
    above 128 vertices, 6 of two small hulls.  The lifts and slides are those of tests/test_gpu_hulls.py: candidate c reaches GAPS[c] at the
    sample TOUCH[c] and its neighbours are millimetres apart, so that few evaluations enter the facet pass.
    Returns (topo, hulls, pairs, q, emulation (S, P), scale (S, P), facet pass entered (S, P), GJK iterations (S, P))."""
    from scipy.spatial.transform import Rotation

    from flobaroid_amd.collision import Hull

    topo = hs.turned_gantry("apex_down")
    R = hs.TURNS["apex_down"]
    rng = np.random.default_rng(33)
    K = ls.kuka_hulls()
    shift = (0.0625, -0.03125)
    z3 = np.zeros(3)
    cols = [(ls.shape("prism400"), ls.shape("sphere257"), shift), (ls.shape("sphere1024"), ls.shape("sphere256"), None),
            (ls.shape("prism130"), ls.shape("cone512"), shift), (K["lwr_base_link"], K["lwr_6_link"], (0.0, 0.0)),
            (Hull("bed", hs.box([0.25, 0.25, 0.25]), z3), Hull("carriage", hs.cone(127, 0.25, 0.5), z3), shift),
            (Hull("bed", hs.wedge(0.25, 0.5, 0.25, "y"), z3), Hull("carriage", hs.wedge(0.25, 0.5, 0.25, "x"), z3), shift)]
    bed, car = [], []
    for k, (A, B, xy) in enumerate(cols):
        va, wb = A.vertices, B.vertices @ R.T
        ia, ib = int(np.argmax(va[:, 2])), int(np.argmin(wb[:, 2]))
        if xy is None:  # B's lowest vertex over A's highest
            xy = va[ia, :2] - wb[ib, :2]
        w = np.array([1.5 * k + xy[0], xy[1], (va[ia, 2] - wb[ib, 2]) - (0.5 + LIFT)])
        bed.append(ls.on(A, "bed", np.array([0.25 + 1.5 * k, 0.0, 0.0])))
        car.append(ls.on(B, "carriage", R.T @ w))
    wall = Hull(None, hs.box([4.5, 0.25, 0.25]), np.array([4.0, 0.625, 0.875]), Rotation.from_euler("xyz", [0.4, 0.05, 0.1]).as_matrix(), "wall")
    hl = [car[2], bed[0], wall, car[0], bed[3], bed[1], car[3], car[1], bed[2], bed[5], car[4], bed[4], car[5]]
    at = {id(h): i for i, h in enumerate(hl)}
    pairs = [(at[id(a)], at[id(b)]) for a, b in zip(bed, car)]
    pairs += [(at[id(bed[i])], at[id(car[j])]) for i, j in ((0, 2), (2, 0), (4, 0), (4, 5), (5, 4))]
    pairs += [((at[id(wall)], at[id(b)]) if k % 2 else (at[id(b)], at[id(wall)])) for k, b in enumerate(car)]
    pairs = np.array([pairs[i] for i in rng.permutation(len(pairs))], dtype=np.int32)
    nv = np.array([len(h.vertices) for h in hl])
    big = (nv[pairs] > SMALL).any(axis=1)
    assert len(pairs) == 17 and big.sum() == 11 and len(pairs) % BATCH != 0 and (np.diff(pairs[:, 0]) < 0).any()
    q = np.zeros((len(GAPS) * TT, 2))
    for c, (gap, k0) in enumerate(zip(GAPS, TOUCH)):
        i = np.arange(TT) - k0
        q[c * TT:(c + 1) * TT, 0] = (LIFT + gap) + np.where(i < 0, -i * 2.0 ** -9, i * 3.0 * 2.0 ** -10)
        q[c * TT:(c + 1) * TT, 1] = np.where(i < 0, i * 2.0 ** -7, i * 3.0 * 2.0 ** -9)
    emu, scale, facet, iters = emulate(topo, False, hl, pairs, q, True)
    return topo, hl, pairs, q, emu, scale, facet, iters


def emulate(topo, floating, hulls, pairs, q, mode):
    """(dist, scale, facet pass entered, GJK iterations) (S, P): the frames of the library's own lane walk on the CPU (tests/emul/hull_emul.cpp,
    through four-vertex stand-ins on the same links: a frame does not depend on the vertices), then fbr_hull_large_distance for a pair
    with a hull above 128 vertices and fbr_hull_distance for the others, as fbr_candidate_hull_distances deals them out"""
    from flobaroid_amd.collision import Hull

    tetra = Hull("t", np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), np.zeros(3))
    stand = [ls.on(tetra, h.link_name, h.offset, h.rot, h.name) for h in hulls]
    fr = emul_eval(topo, floating, stand, np.zeros((0, 2), dtype=np.int32), q, None, None, mode)[0]
    S, P = len(q), len(pairs)
    dist, scale, facet, iters = np.zeros((S, P)), np.zeros((S, P)), np.zeros((S, P), dtype=bool), np.zeros((S, P), dtype=np.int64)
    for k, (a, b) in enumerate(pairs):
        A, B = hulls[a], hulls[b]
        args = (A, B, fr[:, a, :9], fr[:, a, 9:], fr[:, b, :9], fr[:, b, 9:])
        dist[:, k], iters[:, k], facet[:, k] = large_distance(*args, True) if max(len(A.vertices), len(B.vertices)) > SMALL else emul_distance(*args)
        scale[:, k] = hr.pair_scale(fr[:, a, 9:], A.diameter, fr[:, b, 9:], B.diameter)
    return dist, scale, facet, iters


def minima(emu, scale, C):
    """(val, idx, bar, decided) (C, P): the emulation's minima, 32 eps x scale at the winning sample, and whether the runner-up lies more
    than 100 bars above the minimum (the index is asserted there)"""
    val, idx = hr.candidate_minimum(emu, C, 1)
    e3, s3 = emu.reshape(C, -1, emu.shape[1]), scale.reshape(C, -1, emu.shape[1])
    bar = 32.0 * EPS * np.take_along_axis(s3, idx[:, None, :], axis=1)[:, 0]
    runner = np.sort(e3, axis=1)[:, 1]
    return val, idx, bar, runner - val > 100.0 * bar


def test_large_shapes_on_the_gantry_against_the_emulation():
    topo, hl, pairs, q, emu, scale, facet, iters = large_gantry_case()
    C = len(GAPS)
    val, idx, bar, decided = minima(emu, scale, C)
    print(f"large gantry: {len(hl)} hulls of {sorted({len(h.vertices) for h in hl})} vertices, {len(pairs)} pairs; {facet.mean():.4f} of the evaluations enter the "
          f"facet pass; GJK iterations mean {iters.mean():.2f}, most {iters.max()}; {int((~decided).sum())} of {decided.size} columns excluded for a near tie; "
          f"minima <= 0: {(val <= 0).sum()} of {val.size}")
    assert (~decided).mean() <= 0.05 and (val <= 0).sum() >= 6 and (val > 0).sum() >= 6 and iters.max() < 64 and 0 < facet.mean() < 0.1
    eng = _engine(topo, False)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, large=True)
    a, b = _call(eng, q, C, False), _call(eng, q, C, True)
    err = np.abs(a["dist"] - val)
    print(f"large gantry: max |device - emulation| = {err.max():.3e} = {(err / bar).max():.3f} bars (smallest bar {bar.min():.3e}); "
          f"device == emulation in {(a['dist'] == val).mean():.3f} of the columns")
    assert np.all(err <= bar)
    assert np.array_equal(a["idx"][decided], idx[decided])
    assert _same(a, b) and _same(b, _call(eng, q, C, True))  # host and device states, a second run
    eng2 = _engine(topo, False, options={"chunk_samples": 64})
    eng2.set_hulls(hl, pairs, offset_in_link_axes=True, large=True)
    assert _same(a, _call(eng2, q, C))  # one block a launch
    for k in range(C):  # a candidate alone gives the bits of its row
        one = _call(eng, q[k * TT:(k + 1) * TT], 1)
        assert one["dist"].tobytes() == a["dist"][k:k + 1].tobytes() and one["idx"].tobytes() == a["idx"][k:k + 1].tobytes()
    # every pair through the large kernel: equal values, the same winners
    eng.set_option("hull_large_all", 1)
    c = _call(eng, q, C)
    assert np.array_equal(c["dist"], a["dist"]) and np.array_equal(c["idx"], a["idx"])
    eng.close()
    eng2.close()


def test_small_pairs_of_a_mixed_set_return_the_bytes_of_set_hulls():
    topo, hl, pairs, q, *_ = large_gantry_case()
    nv = np.array([len(h.vertices) for h in hl])
    small = ~(nv[pairs] > SMALL).any(axis=1)
    keep = np.nonzero(nv <= SMALL)[0]
    new_of = {int(h): i for i, h in enumerate(keep)}
    assert small.sum() == 6 and 0 < len(keep) < len(hl)
    eng = _engine(topo, False)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, large=True)
    mixed = _call(eng, q, len(GAPS))
    eng.set_hulls([hl[h] for h in keep], np.array([[new_of[int(a)], new_of[int(b)]] for a, b in pairs[small]], dtype=np.int32), offset_in_link_axes=True)
    alone = _call(eng, q, len(GAPS))
    assert np.ascontiguousarray(mixed["dist"][:, small]).tobytes() == alone["dist"].tobytes()
    assert np.array_equal(mixed["idx"][:, small], alone["idx"]) and (alone["dist"] <= 0).any()
    eng.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_large_set_in_place():
    from flobaroid_amd._lib import FbrError
    from flobaroid_amd.collision import Hull

    topo, hl, pairs, q, *_ = large_gantry_case()
    C, P = len(GAPS), len(pairs)
    eng = _engine(topo, False)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, large=True)
    want = _call(eng, q, C)
    over = Hull("bed", hs.fibonacci_sphere(1025, 0.25), np.zeros(3))
    big = int(np.argmax([len(h.vertices) > SMALL for h in hl]))
    st, smp = {"q": q}, np.zeros((C, P), dtype=np.int64)
    tris = hl[big].vertices[:3][None]
    for why, call, msg in (("1025 vertices", lambda: eng.set_hulls([over] + hl[1:], pairs, large=True), "1025 vertices"),
                           ("130 vertices through set_hulls", lambda: eng.set_hulls([ls.on(ls.shape("prism130"), "bed")] + [h for h in hl if len(h.vertices) <= SMALL], []), "130 vertices"),
                           ("the large set through set_hulls", lambda: eng.set_hulls(hl, pairs, offset_in_link_axes=True), "vertices \\(4 to 128\\)"),
                           ("meshes on a large set", lambda: eng.set_hull_meshes({big: tris}), f"hull {big} of the set has {len(hl[big].vertices)} vertices"),
                           ("hull gradients", lambda: eng.hull_distance_gradients(st, C, smp), f"hull {big} of the set has {len(hl[big].vertices)} vertices"),
                           ("mesh gradients", lambda: eng.mesh_distance_gradients(st, C, smp), f"hull {big} of the set has {len(hl[big].vertices)} vertices")):
        with pytest.raises(FbrError, match="code -1") as e:
            call()
        assert __import__("re").search(msg, str(e.value)), (why, str(e.value))
        assert _same(_call(eng, q, C), want), why
    with pytest.raises(ValueError, match="large=True"):  # the binding: meshes= with large=True
        eng.set_hulls(hl, pairs, offset_in_link_axes=True, meshes={big: tris}, large=True)
    assert _same(_call(eng, q, C), want)
    # either call replaces the set the other installed
    small = [h for h in hl if len(h.vertices) <= SMALL and h.link_name]
    eng.set_hulls(small, [[0, 1]])
    assert eng.candidate_hull_distances(st, C, 1)["dist"].shape == (C, 1)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, large=True)
    assert _same(_call(eng, q, C), want)
    eng.close()


# ---- KUKA LWR4 --------------------------------------------------------------------------------------------------------------------------------
def restate_block(topo, cs, q, config):
    """The reference's collision loop for ONE candidate of a fixed-base robot, sample by sample, on the Qhull restatement: restate_hull_block of
    tests/test_hulls.py with the world poses formed once and hull_restatement.hull_distance called pair by pair (pair_distances derives
    every hull's diameter anew at each call, seconds a candidate with hulls of 600 vertices).  (g (P,), {pair: the reference's argmin})"""
    hulls, P = as_tuples(topo, cs["hulls"]), len(cs["pair_names"])
    pairs = cs["hull_pairs"][cs["columns"][:, 1]]  # in the order of pair_names
    mode = bool(cs.get("offset_in_link_axes", False))
    T, ns = q.shape[0], int(config.get("transitionCollisionSamples", 10))
    rows = [(q[i], i) for i in range(0, T, int(config.get("collisionCheckStep", 3)))]
    if config.get("transitionDuration", 3.0) > 0 and ns > 0:
        for qb in (q[0], q[-1]):
            for j in range(ns):
                tau = (j + 1) / (ns + 1)
                rows.append(((10 * tau**3 - 15 * tau**4 + 6 * tau**5) * qb, None))
    R, c = hr.hull_world(topo, hulls, np.array([r[0] for r in rows]), False, None, None, mode)
    g, main = np.full(P, 1e10), {}
    for s, (_, i) in enumerate(rows):
        for k, (a, b) in enumerate(pairs):
            d = hr.hull_distance(R[s, a], c[s, a], hulls[a][3], R[s, b], c[s, b], hulls[b][3]) - cs["margins"][k]
            if d < g[k]:
                g[k] = d
                if i is not None:
                    main[k] = i
    return g, main


def test_kuka_convex_collision_block_and_the_gradient_refusal():
    """Fixed base, the eight hulls of the fixture and the floor of world_kuka.urdf: the floor against lwr_2_link .. lwr_7_link and
    lwr_base_link against lwr_7_link (the pairs Qhull restates in milliseconds; every one has a hull above 128 vertices).  C = 2, T = 64,
    collisionCheckStep 1, transitions on; small amplitudes about a bent posture, the floor lifted under the wrist of the first sample of
    the first candidate, so that few evaluations overlap.  The bar: 32 eps x scale of the pair, the smaller term of the project's rule."""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from flobaroid_amd.collision import collision_set, world_hulls_from_urdf
    from test_gpu_box_objectives import _cols

    topo = load_topo("kuka_lwr4")
    K = ls.kuka_hulls()
    eng = Engine(topo, floating=False)
    rng = np.random.default_rng(35)
    n, C, T, freq = topo.num_dofs, 2, 64, 100.0
    arm = [f"lwr_{i}_link" for i in range(1, 8)]
    config = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0, "collisionCheckStep": 1,
              "transitionDuration": 3.0, "transitionCollisionSamples": 1, "collisionMode": "convex", "worldCollisionMargin": 0.01,
              "ignoreLinkPairsForCollision": [[a, b] for i, a in enumerate(arm) for b in arm[i + 1:]] + [["lwr_base_link", a] for a in arm[:6]]
              + [["ground_link", "lwr_base_link"], ["ground_link", "lwr_1_link"]]}
    posture = np.array([0.3, 1.9, -0.4, -1.2, 0.5, 0.9, 0.2])
    cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.02 for _ in range(n)], [rng.standard_normal(2) * 0.02 for _ in range(n)],
                                      posture + rng.uniform(-0.02, 0.02, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    st = exc.candidate_states(eng, cands, T, freq)
    q = _host(st)["q"]
    wh = world_hulls_from_urdf(os.path.join(GOLDEN, "urdf", "world_kuka.urdf"), "geometric")
    tup7 = as_tuples(topo, [K["lwr_7_link"]])
    R7, c7 = hr.hull_world(topo, tup7, q[:1], False, None, None, False)
    low = float((c7[0, 0] + K["lwr_7_link"].vertices @ R7[0, 0].T)[:, 2].min())
    wh["ground_link"].offset = wh["ground_link"].offset + np.array([0.0, 0.0, low - 0.012])  # its top 2 mm inside the margin below the flange
    cs = collision_set(topo, {}, config, hulls=K, world_hulls=wh)
    P = len(cs["pair_names"])
    assert np.all(cs["columns"][:, 0] == 2) and 6 <= P <= 12, cs["pair_names"]
    nv = np.array([len(h.vertices) for h in cs["hulls"]])
    assert (nv[cs["hull_pairs"]] > SMALL).any(axis=1).all() and ("lwr_6_link", 793) in exc._large_hulls(cs)
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    cols = _cols(eng, topo, False)
    base = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config)
    full = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, collision=cs)
    n0 = base["g"].shape[1]
    assert full["g"].shape == (C, n0 + P) and full["g"][:, :n0].tobytes() == base["g"].tobytes()
    tup = as_tuples(topo, cs["hulls"])
    pr = cs["hull_pairs"][cs["columns"][:, 1]]
    diam = np.array([h.diameter for h in cs["hulls"]])
    for k in range(C):
        s = slice(k * T, (k + 1) * T)
        g, argmin = restate_block(topo, cs, q[s], config)
        _, cen = hr.hull_world(topo, tup, q[s], False, None, None, bool(cs.get("offset_in_link_axes", False)))
        bar = 32.0 * EPS * (np.linalg.norm(cen[:, pr[:, 1]] - cen[:, pr[:, 0]], axis=2).min(axis=0) + diam[pr[:, 0]] + diam[pr[:, 1]])
        err = np.abs(full["g"][k, n0:] - g)
        print(f"KUKA candidate {k}: convex collision block max |delta| {err.max():.2e} = {(err / bar).max():.3f} bars (smallest bar {bar.min():.2e}); "
              f"{int((g < 0).sum())} of {P} pairs in collision")
        assert np.all(err <= bar)
        assert all(full["ag_cache"]["collision_argmin_idx"][k, p] == argmin.get(p, -1) for p in range(P)), k
    blk = full["g"][:, n0:]
    assert (blk < 0).any() and (blk > 0).any()
    for kw in ({"hull_gradient": True}, {}):
        with pytest.raises(ValueError, match=r"lwr_6_link \(793 vertices\)"):
            exc.candidate_gradients_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, dopt_scale=1.0, collision=cs, **kw)
    eng.close()
