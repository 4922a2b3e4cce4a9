"""fbr_model_set_hull_meshes / fbr_candidate_hull_distances with triangle meshes on the device against the g++ emulation of the same text
(tests/emul/mesh_emul.cpp on the frames of tests/emul/hull_emul.cpp) and the restatement of tests/mesh_restatement.py.

The bar of a (candidate, pair) is, at the restatement's winning sample, the larger of 10 x the largest deviation the emulation shows against
the restatement on the same inputs, and 32 eps x the pair's scale |cB - cA| + diam hull A + diam hull B.  Before the device is asked, on
the CPU: every checked sample of every pair is out of the grey zone (its signed restatement value more than 100 bars from 0: a clear
intersection or a clear gap), the runner-up of a positive minimum lies more than 100 bars above it, and a mesh pair that intersects at
all is won by its FIRST intersecting sample (0.0, strict <) -- so every index is decided.  The emulation gives the same bits with its
culling off.  The references are computed once a case and shared by its tests.

(a) the floating left arm under the crane (tests/test_gpu_hulls.py), LShr a box, fullMeshLinks the hand (SoftHandOpen.STL, 100
triangles) and the forearm (Forearm.STL, 70): mesh-hull, mesh-box, mesh-world and the mesh-mesh pair beside plain hull pairs; C = 3,
T = 200, step 3.  Its nine pairs are a SUBSET of what collision_set builds for this arm, one of each kind and five plain ones, and LShr is
made a box to have a mesh-box pair: chosen for the restatement's cost (below), not for the device's.  (b) walkman_apriori.urdf, the cage around the torso (ProtectionSystem.STL) as a mesh against hulls of the left arm,
every link without a fixture mesh a box; C = 2, T = 67, step 1; the states hold poses in which an arm link is more than 1 mm inside the
cage's hull and more than 1 mm from its triangles.  (c) the gantry of tests/hull_shapes.py with exact poses: a mesh apex on a mesh
face, on a solid face, a solid apex on a mesh face, at gaps 1e-9, 0, -1e-9 reached in one lane that wins its pair.  (d) one block a
launch, each candidate alone, the pair list and the mesh list shuffled: the same bits.  T = 67 leaves 3 live lanes in the last block.

Seen on an MI355X: (a) |device - emulation| <= 1.2e-16 = 0.014 bars (not the same bits: the frames of the device's walk differ in the last
place, as for the hulls), |device - restatement| <= 2.2e-16 (emulation - restatement 6.1e-16, smallest bar 6.1e-15); (b) 1.1e-16 = 0.011
bars, 3.3e-16; (c) the emulation's bits on every pair, the contacts 1.000000082740371e-09 (the gap as the lift's rounding leaves it),
0.0, 0.0; 10 GJK iterations at most ("Triangle meshes").  The Qhull restatement of a triangle against a hull takes half a
millisecond, 240 of them a sample in (a): the references took 44 s, 22 s and 6 s on the CPUs they have run on, once a session."""
import functools
import os

import numpy as np
import pytest

import hull_restatement as hr
import hull_shapes as hs
import mesh_restatement as mr
import test_meshes as tm
from common import GOLDEN, load_topo, random_states
from test_gpu_boxes import _dev, _engine, _host
from test_hulls import EPS, as_tuples, emul_eval, left_arm_hulls

pytestmark = pytest.mark.gpu
URDF = os.path.join(GOLDEN, "urdf")


def is_mesh_pair(pairs, meshes):
    return np.array([int(a) in meshes or int(b) in meshes for a, b in pairs])


def reference(topo, floating, hulls, meshes, pairs, st, bp, mode, C, T, STEP, free=()):
    """(val, idx, bar, emulation's minima, emulation - restatement) (C, P) the device has to meet, after the assertions on the CPU's side.
    ``free``: (row, pair) entries that are exact contacts by construction and exempt from the grey-zone rule."""
    rows = [c * T + i for c in range(C) for i in range(0, T, STEP)]
    tup = as_tuples(topo, hulls)
    q, rpy = st["q"], st.get("rpy") if floating else None
    R, cen = hr.hull_world(topo, tup, q, floating, rpy, bp if floating else None, mode)
    signed, scale = mr.pair_signed(R, cen, tup, meshes, pairs, rows)
    want = mr.pair_distances(signed, pairs, meshes)
    fr, hull_emu, _ = emul_eval(topo, floating, hulls, pairs, q, rpy, bp if floating else None, mode)
    emu, sa, sb = tm.both(fr, hulls, meshes, pairs)
    mp = is_mesh_pair(pairs, meshes)
    assert emu[:, ~mp].tobytes() == hull_emu[:, ~mp].tobytes()  # (plain pairs: the hull routine)
    fin = np.isfinite(want)
    dev = float(np.abs(emu - want)[fin].max())
    bar = np.maximum(10.0 * dev, 32.0 * EPS * scale)
    grey = fin & (np.abs(signed) <= 100.0 * bar) & mp[None, :]
    for r, k in free:
        grey[r, k] = False
    assert not grey.any(), f"mesh pairs in the grey zone at (row, pair) {np.argwhere(grey)[:5].tolist()}: change the seed"
    val, idx = hr.candidate_minimum(np.where(fin, want, np.inf), C, STEP)
    eval_, eidx = hr.candidate_minimum(emu, C, STEP)
    w3 = np.where(fin, want, np.inf).reshape(C, T, -1)[:, ::STEP]
    cbar = np.take_along_axis(bar.reshape(C, T, -1)[:, ::STEP], (idx // STEP)[:, None, :], axis=1)[:, 0]
    runner = np.sort(w3, axis=1)[:, 1]
    decided = (runner - val > 100.0 * cbar) | ((val == 0.0) & mp[None, :])
    assert decided.all(), "a runner-up lies within 100 bars of a minimum: change the seed"
    assert np.array_equal(eidx, idx) and np.all(np.abs(eval_ - val) <= cbar)
    assert np.all(val[:, mp] >= 0.0)
    print(f"mesh reference: {len(hulls)} hulls, {len(meshes)} meshes, {len(pairs)} pairs ({int(mp.sum())} with a mesh), {len(rows)} samples; "
          f"emulation - restatement {dev:.3e}; smallest bar {cbar.min():.3e}; mesh minima at 0.0: {int((val[:, mp] == 0).sum())} of {val[:, mp].size}; "
          f"the culling removed {1 - sa[0] / max(sb[0], 1):.2%} of {sb[0]} triangle evaluations; most GJK iterations {max(sa[2], sb[2])}")
    return val, idx, cbar, eval_, dev


def call(eng, st, bp, C, STEP, device, rows=slice(None)):
    s2 = {k: np.ascontiguousarray(st[k][rows]) for k in ("q", "rpy") if k in st}
    b2 = None if bp is None else np.ascontiguousarray(bp[rows])
    if device:
        import torch

        got = eng.candidate_hull_distances(_dev(s2), C, STEP, base_pos=None if b2 is None else torch.from_numpy(b2).cuda())
    else:
        got = eng.candidate_hull_distances(s2, C, STEP, base_pos=b2)
    return _host(got)


def within(got, ref, why):
    val, idx, bar, emu, dev = ref
    err, err2 = np.abs(got["dist"] - emu), np.abs(got["dist"] - val)
    print(f"mesh case {why}: max |device - emulation| = {err.max():.3e} = {(err / bar).max():.3f} bars ({'the same bits' if err.max() == 0 else 'not the same bits'}), "
          f"|device - restatement| = {err2.max():.3e} (emulation - restatement {dev:.3e}; smallest bar {bar.min():.3e})")
    assert np.array_equal(got["idx"], idx), why
    assert np.all(err <= bar) and np.all(err2 <= bar), why


def same(a, b):
    return a["dist"].tobytes() == b["dist"].tobytes() and a["idx"].tobytes() == b["idx"].tobytes()


# ---- (a) the left arm under the crane -------------------------------------------------------------------------------------------------------------
C, T, STEP = 3, 200, 3


@functools.lru_cache(maxsize=None)
def left_arm_case():
    from flobaroid_amd.collision import Box, hull_from_box, world_hulls_from_urdf

    rng = np.random.default_rng(12)
    topo, (hulls, _) = left_arm_hulls()
    ms = tm.fixture_meshes()
    b = hulls["LShr"].bounds
    hulls["LShr"] = hull_from_box(Box("LShr", 0.5 * (b[1] - b[0]), hulls["LShr"].offset + 0.5 * (b[0] + b[1])))
    wh = world_hulls_from_urdf(os.path.join(URDF, "world_walkman_suspended.urdf"), "geometric")
    hl = [hulls[n] for n in topo.link_names if n in hulls] + list(wh.values())
    name = [h.link_name or h.name for h in hl]
    at = {n: i for i, n in enumerate(name)}
    meshes = {at["LSoftHandLink"]: ms["LSoftHandLink"].triangles, at["LForearm"]: ms["LForearm"].triangles}
    st = random_states(topo, C * T, rng, True, use_limits=True)
    st["rpy"] = rng.uniform(-0.6, 0.6, (C * T, 3))
    bp = wh["crane_tip"].offset + rng.standard_normal((C * T, 3)) * 0.15
    # the mesh-mesh pair, mesh-hull, mesh-box, mesh-world, and five plain hull pairs (the Qhull restatement of a triangle against a hull takes
    # half a millisecond: 240 of them a sample)
    want = [("LForearm", "LSoftHandLink"), ("LShp", "LForearm"), ("LShr", "LForearm"), ("LSoftHandLink", "crane_arm"),
            ("Waist", "LElb"), ("LShp", "LElb"), ("LShr", "LWrMot2"), ("LShy", "crane_tip"), ("LElb", "crane_arm")]
    pairs = np.array(sorted((at[a], at[b]) for a, b in want), dtype=np.int32)
    return topo, hl, meshes, pairs, st, bp, reference(topo, True, hl, meshes, pairs, st, bp, True, C, T, STEP)


def test_left_arm_with_the_hand_and_the_forearm_as_meshes():
    topo, hl, meshes, pairs, st, bp, ref = left_arm_case()
    mp = is_mesh_pair(pairs, meshes)
    assert mp.sum() == 4 and (~mp).sum() == 5
    eng = _engine(topo, True)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True)
    plain = call(eng, st, bp, C, STEP, True)
    eng.set_hull_meshes(meshes)
    a = call(eng, st, bp, C, STEP, False)
    b = call(eng, st, bp, C, STEP, True)
    within(a, ref, "left arm, host states")
    within(b, ref, "left arm, device states")
    assert same(a, b)
    # the plain hull pairs return the bits they return from the set without meshes; the mesh pairs are never below their hulls' distance
    assert a["dist"][:, ~mp].tobytes() == plain["dist"][:, ~mp].tobytes() and np.array_equal(a["idx"][:, ~mp], plain["idx"][:, ~mp])
    assert np.all(a["dist"][:, mp] >= 0.0) and np.all(a["dist"][:, mp] >= plain["dist"][:, mp] - ref[2][:, mp])
    # set_hulls(meshes=) is the same call; a later set_hulls without meshes clears them; an empty mesh list clears them
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, meshes=meshes)
    assert same(call(eng, st, bp, C, STEP, True), a)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True)
    assert same(call(eng, st, bp, C, STEP, True), plain)
    eng.set_hull_meshes(meshes)
    eng.set_hull_meshes({})
    assert same(call(eng, st, bp, C, STEP, True), plain)


def test_variants_give_the_same_bits():
    """(d): one block a launch, each candidate alone, the pair list shuffled (the same columns), the mesh list shuffled"""
    topo, hl, meshes, pairs, st, bp, ref = left_arm_case()
    eng = _engine(topo, True)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, meshes=meshes)
    a = call(eng, st, bp, C, STEP, True)
    within(a, ref, "left arm")
    eng2 = _engine(topo, True, options={"chunk_samples": 64})
    eng2.set_hulls(hl, pairs, offset_in_link_axes=True, meshes=meshes)
    assert same(call(eng2, st, bp, C, STEP, True), a)
    for k in range(C):
        one = call(eng, st, bp, 1, STEP, True, slice(k * T, (k + 1) * T))
        assert one["dist"].tobytes() == a["dist"][k:k + 1].tobytes() and one["idx"].tobytes() == a["idx"][k:k + 1].tobytes()
    perm = np.random.default_rng(5).permutation(len(pairs))
    eng.set_hulls(hl, pairs[perm], offset_in_link_axes=True, meshes=meshes)
    b = call(eng, st, bp, C, STEP, True)
    assert b["dist"].tobytes() == np.ascontiguousarray(a["dist"][:, perm]).tobytes() and np.array_equal(b["idx"], a["idx"][:, perm])
    eng.set_hulls(hl, pairs, offset_in_link_axes=True)
    eng.set_hull_meshes(list(meshes.items())[::-1])
    assert same(call(eng, st, bp, C, STEP, True), a)


def test_refused_meshes_leave_the_attachments_in_place():
    from flobaroid_amd._lib import FbrError

    topo, hl, meshes, pairs, st, bp, ref = left_arm_case()
    eng = _engine(topo, True)
    with pytest.raises(FbrError, match="code -1"):  # no hull set
        eng.set_hull_meshes(meshes)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, meshes=meshes)
    a = call(eng, st, bp, C, STEP, True)
    h0, t0 = next(iter(meshes.items()))
    world = next(i for i, h in enumerate(hl) if h.link_name is None)
    for bad in ({len(hl): t0}, [(h0, t0), (h0, t0)], {world: t0}, {h0: t0[:0]}, {h0: t0 * 3.0}, {h0: np.where(np.arange(t0.size).reshape(t0.shape) == 4, np.nan, t0)},
                {h0: np.tile(t0[:1], (257, 1, 1))}):
        with pytest.raises(FbrError, match="code -1"):
            eng.set_hull_meshes(bad)
    assert same(call(eng, st, bp, C, STEP, True), a)
    with pytest.raises(FbrError, match="code -4"):  # FBR_E_UNSUPPORTED: gradients of a set with meshes
        eng.hull_distance_gradients({"q": st["q"], "rpy": st["rpy"]}, C, np.zeros((C, len(pairs)), dtype=np.int64), base_pos=bp)
    eng.set_hull_meshes({})
    got = eng.hull_distance_gradients({"q": st["q"], "rpy": st["rpy"]}, C, np.zeros((C, len(pairs)), dtype=np.int64), base_pos=bp)
    assert np.isfinite(_host(got)["dist"]).all()


# ---- (b) the cage around the torso ------------------------------------------------------------------------------------------------------------------
BC, BT = 2, 67
ARM = ("LShp", "LElb", "LForearm")


@functools.lru_cache(maxsize=None)
def cage_case():
    from flobaroid_amd.collision import hulls_from_urdf, meshes_from_urdf

    topo = load_topo("walkman_apriori")
    urdf = os.path.join(URDF, "walkman_apriori.urdf")
    hulls, box_links = hulls_from_urdf(urdf, topo.link_names, x_std=topo.x_std(), cube_size=0.1)
    cage = meshes_from_urdf(urdf, ["TorsoProtections"])["TorsoProtections"]
    assert len(box_links) > 10 and "TorsoProtections" not in box_links and all(n not in box_links for n in ARM)
    keep = ["TorsoProtections", *ARM, "LHipMot", "NeckPitch", "RHipMot"]
    hl = [cage.hull] + [hulls[n] for n in keep[1:]]
    assert all(len(hulls[n].vertices) == 8 and n in box_links for n in keep[4:])  # (boxes: no fixture mesh)
    meshes = {0: cage.triangles}
    # the cage against three hulls of the arm and a box; four plain pairs
    pairs = np.array([(0, 1), (0, 2), (0, 3), (0, 4), (1, 4), (2, 5), (3, 6), (1, 6)], dtype=np.int32)
    # Built on the host.  Candidate 0: random states within the limits (the shoulder link LShp sits inside the cage's hull in every pose).
    # Candidate 1: small motions about state 1862 of 3000 random ones (seed 0), found on the CPU: the forearm reaches through the cage there,
    # 0.19 m inside its hull and 0.08 m from its triangles over the candidate.
    pool = random_states(topo, 3000, np.random.default_rng(0), False, use_limits=True)["q"]
    rng = np.random.default_rng(2)
    st = random_states(topo, BC * BT, rng, False, use_limits=True)
    st["q"][BT:] = pool[1862] + 0.01 * rng.standard_normal((BT, topo.num_dofs))
    ref = reference(topo, False, hl, meshes, pairs, st, None, False, BC, BT, 1)
    # by the restatement: an arm link inside the cage's hull by more than 1 mm, more than 1 mm clear of its triangles
    tup = as_tuples(topo, hl)
    R, cen = hr.hull_world(topo, tup, st["q"], False, None, None, False)
    inside = []
    for c in range(BC):
        for k in range(1, 4):
            s = c * BT + int(ref[1][c, k - 1])
            hd = hr.hull_distance(R[s, 0], cen[s, 0], tup[0][3], R[s, k], cen[s, k], tup[k][3])
            if hd < -1e-3 and ref[0][c, k - 1] > 1e-3:
                inside.append((c, keep[k], hd, float(ref[0][c, k - 1])))
    print(f"cage case: (candidate, link, hull distance, mesh distance) inside the cage's hull and clear of it: {inside}")
    assert {(c, n) for c, n, _, _ in inside} >= {(0, "LShp"), (1, "LForearm")}, "no arm link inside the cage's hull and clear of its triangles"
    return topo, hl, meshes, pairs, st, ref


def test_the_cage_as_a_mesh_against_the_left_arm():
    topo, hl, meshes, pairs, st, ref = cage_case()
    eng = _engine(topo, False)
    eng.set_hulls(hl, pairs)
    plain = call(eng, st, None, BC, 1, True)
    eng.set_hull_meshes(meshes)
    a = call(eng, st, None, BC, 1, False)
    b = call(eng, st, None, BC, 1, True)
    within(a, ref, "cage, host states")
    within(b, ref, "cage, device states")
    assert same(a, b)
    mp = is_mesh_pair(pairs, meshes)
    assert a["dist"][:, ~mp].tobytes() == plain["dist"][:, ~mp].tobytes()
    assert ((plain["dist"][:, mp] < -1e-3) & (a["dist"][:, mp] > 1e-3)).any()  # the hull reports a collision, the mesh a clearance


# ---- (c) exact contacts on the gantry -----------------------------------------------------------------------------------------------------------------
GAPS = (1e-9, 0.0, -1e-9)
TOUCH = (5, 63, 65)  # the sample that reaches the gap: a lane of the full block, its last lane, the block of 3
LIFT = 0.25
GT = 67


@functools.lru_cache(maxsize=None)
def gantry_case():
    """three columns, 1.5 m apart in x: a cube on the bed under a tetrahedron, apex down, on the carriage, whose apex is on the cube's top
    face when the lift is 0.25 and the slide 0 -- mesh on mesh, solid cube under a mesh, mesh under a solid tetrahedron"""
    from flobaroid_amd.collision import Hull

    topo = hs.gantry()
    cube = hs.box([0.25, 0.25, 0.25])
    tet = np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.25], [-0.125, 0.125, 0.25], [-0.125, -0.125, 0.25]])
    cube_t = tm.box_triangles([0.25, 0.25, 0.25])
    tet_t = np.array([[tet[0], tet[1], tet[2]], [tet[0], tet[2], tet[3]], [tet[0], tet[3], tet[1]], [tet[1], tet[3], tet[2]]])
    bed = [Hull("bed", cube, np.array([0.25 + 1.5 * k, 0.0, 0.0])) for k in range(3)]
    car = [Hull("carriage", tet, np.array([1.5 * k + 0.0625, -0.03125, -0.25 - LIFT])) for k in range(3)]
    hl = [car[1], bed[0], car[0], bed[2], bed[1], car[2]]
    at = {id(h): i for i, h in enumerate(hl)}
    meshes = {at[id(bed[0])]: cube_t, at[id(car[0])]: tet_t, at[id(car[1])]: tet_t, at[id(bed[2])]: cube_t}
    # the three contacts, a far mesh-mesh pair, a far mesh-solid pair and a plain one
    pairs = [(bed[0], car[0]), (bed[1], car[1]), (bed[2], car[2]), (bed[0], car[1]), (bed[2], car[1]), (bed[1], car[2])]
    pairs = np.array([(at[id(a)], at[id(b)]) for a, b in pairs], dtype=np.int32)[np.random.default_rng(8).permutation(6)]
    q = np.zeros((len(GAPS) * GT, 2))
    for c, (gap, k0) in enumerate(zip(GAPS, TOUCH)):
        i = np.arange(GT) - k0
        q[c * GT:(c + 1) * GT, 0] = (LIFT + gap) + np.where(i < 0, -i * 2.0 ** -9, i * 3.0 * 2.0 ** -10)
        q[c * GT:(c + 1) * GT, 1] = np.where(i < 0, i * 2.0 ** -7, i * 3.0 * 2.0 ** -9)
    st = {"q": q}
    contact = [int(np.nonzero((pairs == (at[id(a)], at[id(b)])).all(axis=1))[0][0]) for a, b in zip(bed, car)]
    free = [(c * GT + k0, k) for c, k0 in enumerate(TOUCH) for k in contact]
    ref = reference(topo, False, hl, meshes, pairs, st, None, False, len(GAPS), GT, 1, free=free)
    val, idx = ref[0][:, contact], ref[1][:, contact]
    assert np.all(idx == np.array(TOUCH)[:, None]) and np.all(np.abs(val[0] - 1e-9) <= 1e-14) and np.all(val[1:] <= 64 * EPS)
    assert np.all(ref[3][0, contact] > 0) and np.all(ref[3][1:, contact] == 0.0)  # the emulation: exactly 0.0 at the gaps 0 and -1e-9
    return topo, hl, meshes, pairs, st, ref, contact


def test_exact_contacts_on_the_gantry():
    topo, hl, meshes, pairs, st, ref, contact = gantry_case()
    eng = _engine(topo, False)
    eng.set_hulls(hl, pairs, meshes=meshes)
    a = call(eng, st, None, len(GAPS), 1, False)
    b = call(eng, st, None, len(GAPS), 1, True)
    assert same(a, b)
    val, idx, bar, emu, dev = ref
    d = a["dist"][:, contact]
    print(f"gantry: the contact pairs (mesh on mesh, solid under mesh, mesh under solid) by gap: {dict(zip(GAPS, d.tolist()))}; "
          f"max |device - emulation| over all pairs {np.abs(a['dist'] - emu).max():.3e}")
    assert np.all(a["idx"][:, contact] == np.array(TOUCH)[:, None])
    assert np.all(np.abs(d[0] - 1e-9) <= bar[0, contact]) and np.all(d[1] == 0.0) and np.all(d[2] == 0.0)
    assert np.array_equal(a["idx"], idx) and np.all(np.abs(a["dist"] - emu) <= bar)
