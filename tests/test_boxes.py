"""Oriented-box collision distances off the GPU: the NumPy restatement (tests/box_restatement.py: separating axes + feature enumeration in
world coordinates) is held against two independent yardsticks -- an active-set QP where the boxes are separated, the facets of the
Minkowski-difference hull where they overlap --, the HIP-free text of csrc/fbr_box.h (g++, tests/emul/box_emul.cpp) against the
restatement on the same inputs and on poses of the lane walk, and the host helpers of flobaroid_amd/collision.py against line-by-line
restatements of the reference's functions."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import box_restatement as br
from common import GOLDEN, ROOT, load_topo, random_states, random_topology

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "box_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libbox_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lib = None
EPS = np.finfo(np.float64).eps


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC] + [os.path.join(_CSRC, h) for h in ("fbr_box.h", "fbr_capsule.h", "fbr_math.h", "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _c(a, t=np.float64):
    return np.ascontiguousarray(a, dtype=t)


def emul_distance(RA, cA, hA, RB, cB, hB):
    RA, cA, hA, RB, cB, hB = (_c(x) for x in (RA, cA, hA, RB, cB, hB))
    out = np.zeros(len(RA))
    emul().box_distance(ctypes.c_long(len(RA)), _d(RA), _d(cA), _d(hA), _d(RB), _d(cB), _d(hB), _d(out))
    return out


def emul_eval(topo, floating, boxes, pairs, q, rpy=None, base_pos=None, center_in_link_axes=False):
    """(frames (S, nboxes, 12), dist (S, P)) from the library's own lane walk and box routine on the CPU"""
    parent, dof, jt = _c(topo.parent, np.int32), _c(topo.dof_index, np.int32), _c(topo.joint_type, np.int32)
    rR, rp, ax = _c(topo.rest_R).reshape(-1), _c(topo.rest_p).reshape(-1), _c(topo.axis).reshape(-1)
    link = _c([b[0] for b in boxes], np.int32)
    half = _c([b[1] for b in boxes]).reshape(-1)
    cen = _c([b[2] for b in boxes]).reshape(-1)
    rot = _c([np.eye(3) if b[3] is None else b[3] for b in boxes]).reshape(-1)
    pr = _c(pairs, np.int32).reshape(-1)
    q = _c(q)
    S, P = q.shape[0], pr.size // 2
    rpy = None if rpy is None else _c(rpy)
    bp = None if base_pos is None else _c(base_pos)
    fr, dist = np.zeros((S, len(boxes), 12)), np.zeros((S, P))
    rc = emul().box_eval(topo.num_links, topo.num_dofs, parent.ctypes.data_as(_ip), dof.ctypes.data_as(_ip), _d(rR), _d(rp), _d(ax),
                         jt.ctypes.data_as(_ip), int(floating), len(boxes), link.ctypes.data_as(_ip), _d(half), _d(cen), _d(rot),
                         int(center_in_link_axes), P, pr.ctypes.data_as(_ip), ctypes.c_long(S), _d(q), _d(rpy), _d(bp), _d(fr), _d(dist))
    assert rc == 0
    return fr, dist


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def random_rotations(rng, N):
    q = rng.standard_normal((N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], axis=1)


def random_cases(seed=0, N=400):
    """random rotations, half extents 0.02 .. 0.4, centre offsets of scale 0.15 (first half) and 0.5"""
    rng = np.random.default_rng(seed)
    RA, RB = random_rotations(rng, N), random_rotations(rng, N)
    hA, hB = rng.uniform(0.02, 0.4, (N, 3)), rng.uniform(0.02, 0.4, (N, 3))
    cA = rng.standard_normal((N, 3)) * 0.3
    cB = cA + rng.standard_normal((N, 3)) * np.where(np.arange(N) < N // 2, 0.15, 0.5)[:, None]
    return RA, cA, hA, RB, cB, hB


def parallel_cases():
    """exactly parallel boxes (one common, axis-aligned or random, rotation): face, edge and corner contact, each touching, 1e-7 apart and
    1e-3 deep; [(name, case)]"""
    out = []
    hA, hB = np.array([0.1, 0.2, 0.15]), np.array([0.05, 0.12, 0.3])
    rng = np.random.default_rng(5)
    for rname, R in (("aligned", np.eye(3)), ("turned", random_rotations(rng, 1)[0])):
        for cname, mask in (("face", (1, 0, 0)), ("edge", (1, 1, 0)), ("corner", (1, 1, 1))):
            for gname, gap in (("touch", 0.0), ("gap", 1e-7), ("deep", -1e-3)):
                m = np.array(mask, dtype=float)
                # along the masked axes the boxes are `gap` apart, along the others B is shifted a little but overlaps A's extent
                loc = m * (hA + hB + gap) + (1 - m) * np.array([0.01, -0.02, 0.03])
                out.append((f"{rname}-{cname}-{gname}", (R, np.array([0.3, -0.2, 0.1]), hA, R, np.array([0.3, -0.2, 0.1]) + R @ loc, hB)))
    return out


def _stack(cases):
    return tuple(np.stack([c[i] for c in cases]) for i in range(6))


def all_cases():
    rnd = random_cases()
    par = _stack([c for _, c in parallel_cases()])
    return tuple(np.concatenate([a, b]) for a, b in zip(rnd, par))


# ---- the restatement against its yardsticks ------------------------------------------------------------------------------------------------
def test_restatement_equals_the_qp_and_the_minkowski_hull():
    """separated: |delta| <= 1e-14 against the QP (both are sums of a few dozen roundings of numbers <= 2); overlapping: <= 1e-14 against the
    hull's facet offsets.  Nothing is left out: no cross axis of the cases is nearly parallel, and each class holds a quarter at least."""
    case = random_cases()
    _, len2, _ = br.sat_axes(case[0], case[3])
    assert not ((len2 > 0) & (len2 < 1e-6)).any()
    d = br.box_distance(*case)
    sep = d > 0
    assert sep.mean() >= 0.25 and (~sep).mean() >= 0.25
    qp = br.qp_distance(*(x[sep] for x in case))
    print(f"separated {sep.sum()}: max |restatement - QP| = {np.abs(d[sep] - qp).max():.2e}")
    assert np.abs(d[sep] - qp).max() <= 1e-14
    # the QP also says that every case the separating axes call overlapping is one: its minimum there is zero
    assert br.qp_distance(*(x[~sep] for x in case)).max() <= 1e-14
    worst = 0.0
    for i in np.nonzero(~sep)[0]:
        worst = max(worst, abs(d[i] - br.hull_depth(*(x[i] for x in case))))
    print(f"overlapping {(~sep).sum()}: max |restatement - hull| = {worst:.2e}")
    assert worst <= 1e-14


def test_restatement_on_exactly_parallel_boxes():
    for name, c in parallel_cases():
        d = br.box_distance(*(x[None] for x in c))[0]
        cname, gname = name.split("-")[1:]
        k = {"face": 1, "edge": 2, "corner": 3}[cname]
        if gname == "gap":  # k axes each 1e-7 apart: the distance is the diagonal
            assert abs(d - 1e-7 * np.sqrt(k)) <= 1e-15, name
            assert abs(d - br.qp_distance(*(x[None] for x in c))[0]) <= 1e-15, name
        elif gname == "touch":
            assert abs(d) <= 4 * EPS, name
        else:  # 1e-3 deep along k axes: the minimum translation is along one of them
            assert abs(d + 1e-3) <= 1e-15, name
            assert abs(d - br.hull_depth(*c)) <= 1e-14, name


# ---- the library's text against the restatement --------------------------------------------------------------------------------------------
def emul_deviation(case):
    """largest |emulation - restatement| over the cases, in units of eps * the pair's scale"""
    want, got = br.box_distance(*case), emul_distance(*case)
    assert np.array_equal(np.isnan(want), np.isnan(got))
    ok = ~np.isnan(want)
    return float((np.abs(got - want)[ok] / (EPS * br.pair_scale(case[1], case[2], case[4], case[5])[ok])).max())


def test_library_box_routine_equals_the_restatement():
    """the two work in different frames (world / the first box's): a few roundings of the pair's scale |cB - cA| + |hA| + |hB|"""
    dev = emul_deviation(all_cases())
    print(f"emulation against restatement: {dev:.2f} eps x scale")
    assert dev <= 16.0
    # the sign never differs on the random cases, and a NaN or an infinite input is a NaN
    case = random_cases()
    assert np.array_equal(emul_distance(*case) > 0, br.box_distance(*case) > 0)
    bad = [x[:4].copy() for x in case]
    bad[0][0, 1, 1] = np.nan
    bad[1][1, 0] = np.inf
    bad[4][2, 2] = np.nan
    got = emul_distance(*bad)
    assert np.isnan(got[:3]).all() and np.isfinite(got[3])
    assert np.isnan(br.box_distance(*bad)[:3]).all()


def synthetic_boxes(topo, rng, per_link=1, pad=(0.02, 0.08)):
    """[(link, half, centre, None)]: a box on every link, about the size of the link (the offset of its first child), centre off the origin"""
    L = topo.num_links
    rp = np.asarray(topo.rest_p, dtype=np.float64).reshape(L, 3)
    out = []
    for l in range(L):
        ch = [c for c in range(L) if topo.parent[c] == l]
        ext = np.abs(rp[ch[0]]) if ch else np.zeros(3)
        for _ in range(per_link):
            out.append((l, 0.5 * ext + rng.uniform(pad[0], pad[1], 3), (0.5 * rp[ch[0]] if ch else np.zeros(3)) + rng.uniform(-0.02, 0.02, 3), None))
    return out


def world_boxes_near(rng, centres, count, half=(0.05, 0.4)):
    """``count`` world boxes [( -1, half, centre, rot)] around points drawn from ``centres`` (S, 3)"""
    R = random_rotations(rng, count)
    return [(-1, rng.uniform(half[0], half[1], 3), centres[rng.integers(len(centres))] + rng.standard_normal(3) * 0.2, R[i]) for i in range(count)]


def mixed_pairs(topo, boxes):
    """robot pairs that are not parent and child (sorted by the first box), every robot box against every world box in between"""
    rob = [i for i, b in enumerate(boxes) if b[0] >= 0]
    wld = [i for i, b in enumerate(boxes) if b[0] < 0]
    out = []
    for i in rob:
        li = boxes[i][0]
        for j in rob:
            lj = boxes[j][0]
            if j > i and li != lj and topo.parent[li] != lj and topo.parent[lj] != li:
                out.append((i, j))
        out += [(i, w) for w in wld]
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def _check_walk(topo, floating, boxes, pairs, st, base_pos, mode):
    R, c, h = br.box_world(topo, boxes, st["q"], floating, st.get("rpy"), base_pos, center_in_link_axes=mode)
    want, scale = br.pair_distances(R, c, h, pairs)
    fr, dist = emul_eval(topo, floating, boxes, pairs, st["q"], st.get("rpy") if floating else None, base_pos if floating else None, mode)
    wscale = max(1.0, float(np.abs(c).max()))
    assert np.abs(fr[..., :9].reshape(R.shape) - R).max() <= 1e-12 and np.abs(fr[..., 9:] - c).max() <= 1e-12 * wscale
    # the poses of the two walks differ by roundings of the world coordinates; the distance is 1-Lipschitz in them
    assert np.all(np.abs(dist - want) <= 1e-12 * wscale + 16 * EPS * scale)
    assert (want > 0).mean() >= 0.1 and (want <= 0).mean() >= 0.1
    return dist


@pytest.mark.parametrize("robot,floating", [("threeLinks", False), ("kuka_lwr4", False), ("walkman_left_arm", True)])
@pytest.mark.parametrize("mode", [False, True])
def test_library_walk_on_robots(robot, floating, mode):
    topo = load_topo(robot)
    rng = np.random.default_rng(2)
    boxes = synthetic_boxes(topo, rng)
    S = 120
    st = random_states(topo, S, rng, floating, use_limits=True)
    bp = None
    if floating:
        st["rpy"] = rng.uniform(-0.6, 0.6, (S, 3))
        bp = rng.standard_normal((S, 3)) * 0.1
    _, p = br.link_poses(topo, st["q"], floating, st.get("rpy"), bp)
    boxes += world_boxes_near(rng, np.concatenate([x for x in p]), 4)
    _check_walk(topo, floating, boxes, mixed_pairs(topo, boxes), st, bp, mode)


@pytest.mark.parametrize("seed", [3, 4])
def test_library_walk_random_trees_with_fixed_and_prismatic_joints(seed):
    rng = np.random.default_rng(seed)
    topo = random_topology(rng, int(rng.integers(5, 20)), p_fixed=0.25, branchiness=0.5, p_prismatic=0.3)
    boxes = synthetic_boxes(topo, rng, per_link=2, pad=(0.2, 0.6))  # (links a metre apart: fat boxes overlap often enough)
    fl = bool(seed % 2)
    S = 80
    st = random_states(topo, S, rng, fl)
    bp = rng.standard_normal((S, 3)) * 0.2 if fl else None
    _, p = br.link_poses(topo, st["q"], fl, st.get("rpy"), bp)
    boxes += world_boxes_near(rng, np.concatenate([x for x in p]), 6, half=(0.3, 0.8))
    _check_walk(topo, fl, boxes, mixed_pairs(topo, boxes), st, bp, bool(seed % 2))


# ---- flobaroid_amd/collision.py ------------------------------------------------------------------------------------------------------
def _world(name):
    return os.path.join(GOLDEN, "urdf", f"world_{name}.urdf")


def test_world_boxes_of_the_fixtures_in_both_placements():
    from flobaroid_amd.collision import world_boxes_from_urdf

    want = {"kuka": ["ground_link"], "walkman_fixed": ["ground_link", "seat_link"],
            "walkman_suspended": ["ground_link", "crane_column", "crane_arm", "crane_tip"]}
    for w, links in want.items():
        ref, geo = world_boxes_from_urdf(_world(w)), world_boxes_from_urdf(_world(w), placement="geometric")
        assert list(ref) == links == list(geo)  # (the bare frame "world" is no link of the list)
        for n in links:
            assert ref[n].link_name is None and ref[n].name == n
            assert np.array_equal(ref[n].rot, np.eye(3)) and np.array_equal(geo[n].rot, np.eye(3))
            assert np.array_equal(ref[n].half, geo[n].half) and np.all(ref[n].half > 0)
            assert np.array_equal(ref[n].center, 2.0 * geo[n].center)  # (symmetric boxes: mid = 0, the position is counted twice)
    # the crane arm by hand: joint at (-1.2, 0, 0.25), visual origin (0.8, 0, 0), <box size="2.0 0.10 0.10">
    pos = np.array([-1.2, 0.0, 0.25]) + np.array([0.8, 0.0, 0.0])
    arm = world_boxes_from_urdf(_world("walkman_suspended"))["crane_arm"]
    assert np.array_equal(arm.half, [1.0, 0.05, 0.05])
    assert np.array_equal(arm.center, pos + (np.zeros(3) + pos))  # _getLinkTransform's pos + _getLinkCollisionGeometry's (mid + pos)
    assert np.array_equal(world_boxes_from_urdf(_world("walkman_suspended"), "geometric")["crane_arm"].center, pos)
    assert np.array_equal(world_boxes_from_urdf(_world("kuka"), "geometric")["ground_link"].center, [0, 0, -0.025])
    with pytest.raises(ValueError):
        world_boxes_from_urdf(_world("kuka"), placement="elsewhere")


def test_boxes_from_hulls_and_from_urdf():
    from flobaroid_amd.collision import boxes_from_hulls, boxes_from_urdf

    hulls = {"a": [[[-0.1, -0.2, 0.0], [0.3, 0.2, 0.5]], [0.01, 0.02, 0.03], np.eye(3)],
             "w": [[[-1.0, -1.0, -0.5], [1.0, 1.0, 0.0]], [0.0, 0.5, -1.0], [0.0, 0.0, np.pi / 2]]}
    boxes, world = boxes_from_hulls(hulls, ["a", "b"], scale=0.9)
    b = np.array(hulls["a"][0]) * 0.9
    assert list(boxes) == ["a"] and np.array_equal(boxes["a"].center, 0.5 * (b[0] + b[1]) + np.array(hulls["a"][1]))
    assert np.array_equal(boxes["a"].half, 0.5 * (b[1] - b[0])) and boxes["a"].rot is None
    bw, pw = np.array(hulls["w"][0]), np.array(hulls["w"][1])
    assert list(world) == ["w"] and np.array_equal(world["w"].center, pw + (0.5 * (bw[0] + bw[1]) + pw)) and np.array_equal(world["w"].half, [1, 1, 0.25])
    assert np.abs(world["w"].rot - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])).max() <= 1e-16
    # threeLinks: primitives only; kuka: meshes, reported, and given the cube around the a-priori COM when asked for
    import xml.etree.ElementTree as ET

    for robot in ("threeLinks", "kuka_lwr4"):
        urdf = os.path.join(GOLDEN, "urdf", robot + ".urdf")
        names = [l.attrib["name"] for l in ET.parse(urdf).findall("link")]
        got, mesh = boxes_from_urdf(urdf, names)
        assert not set(got) & set(mesh)
        for l in ET.parse(urdf).findall("link"):
            prim = any(l.find(f"{p}/geometry/{g}") is not None for p in ("visual", "collision") for g in ("box", "cylinder", "sphere"))
            has_mesh = any(l.find(f"{p}/geometry/mesh") is not None for p in ("visual", "collision"))
            assert (l.attrib["name"] in mesh) == has_mesh and (l.attrib["name"] in got) == (prim and not has_mesh)
        if mesh:
            x = np.arange(1, 10 * len(names) + 1, dtype=float)
            cube, _ = boxes_from_urdf(urdf, names, x_std=x, cube_size=0.2, scale=0.5)
            i = names.index(mesh[0])
            assert np.allclose(cube[mesh[0]].half, 0.05) and np.allclose(cube[mesh[0]].center, 0.5 * x[10 * i + 1:10 * i + 4] / x[10 * i])


@pytest.mark.parametrize("robot,world,cfg", [
    ("kuka_lwr4", "kuka", {"worldCollisionMargin": 0.03}),
    ("kuka_lwr4", "kuka", {"ignoreLinksForCollision": ["lwr_2_link"], "ignoreLinkPairsForCollision": [["ground_link", "lwr_4_link"]]}),
    ("walkman_apriori", "walkman_suspended", {"worldCollisionMargin": 0.05, "ignoreCollisionBetweenGroups": [[["LSoftHand", "LWrMot3"], ["crane_arm", "RFoot"]]]}),
    ("walkman_apriori", "walkman_suspended", {"collisionMaxKinematicDistance": 5, "worldCollisionMargin": 0.05}),
])
def test_pairs_and_margins_with_world_links_equal_the_reference_loop(robot, world, cfg):
    from box_collision_restatement import build_collision_pairs
    from flobaroid_amd.collision import Box, Capsule, collision_pairs, collision_set, link_neighbors, world_boxes_from_urdf

    topo = load_topo(robot)
    names = list(topo.link_names)
    wb = world_boxes_from_urdf(_world(world))
    caps = {n: Capsule(n, np.zeros(3), np.array([0, 0, 0.1]), 0.02) for n in names[::2]}   # every other link has a capsule ...
    boxes = {n: Box(n, np.full(3, 0.05), np.zeros(3)) for n in names[:-1]}                  # ... all but the last a box: the last has no geometry
    no_geom = [n for n in names if n not in caps and n not in boxes]
    assert no_geom == [names[-1]] or names[-1] in caps
    want, margins = build_collision_pairs(names, list(wb), link_neighbors(topo), cfg, no_geom)
    assert collision_pairs(topo, caps, cfg, world_links=list(wb), boxes=boxes) == want
    assert any(b in wb for _, b in want) == (cfg.get("collisionMaxKinematicDistance", 0) == 0)  # (the reference's BFS never reaches a world link)
    # without world links the list is today's: the robot pairs of the same geometry
    assert collision_pairs(topo, {**boxes, **caps}, cfg) == [p for p in want if p[1] not in wb]
    for mode in ("capsule", "box"):
        cs = collision_set(topo, caps, dict(cfg, collisionMode=mode), boxes=boxes, world_boxes=wb)
        assert cs["pair_names"] == want and np.array_equal(cs["margins"], margins)
        for (a, b), (which, col) in zip(want, cs["columns"]):
            if which == 0:
                assert mode == "capsule" and a in caps and b in caps
                assert (cs["capsules"][cs["pairs"][col][0]].link_name, cs["capsules"][cs["pairs"][col][1]].link_name) == (a, b)
            else:
                assert mode == "box" or not (a in caps and b in caps)
                ba, bb = (cs["boxes"][i] for i in cs["box_pairs"][col])
                assert (ba.link_name or ba.name, bb.link_name or bb.name) == (a, b)
        assert sorted(cs["columns"][cs["columns"][:, 0] == 1, 1]) == list(range(len(cs["box_pairs"])))
    # a pair that needs a box of a link that has none is refused
    with pytest.raises(ValueError, match="has no box"):
        collision_set(topo, caps, dict(cfg, collisionMode="box"), boxes={names[0]: boxes[names[0]]}, world_boxes=wb)


def test_collision_pairs_without_world_links_are_unchanged():
    from flobaroid_amd.collision import Capsule, collision_pairs, collision_set
    import json

    gold = np.load(os.path.join(GOLDEN, "ref_capsules.npz"))
    for tag in ("kuka_ignore", "walkman_dist5"):
        topo = load_topo(str(gold[f"pairs_{tag}_robot"]))
        cfg = json.loads(str(gold[f"pairs_{tag}_config"]))
        caps = {n: Capsule(n, np.zeros(3), np.array([0, 0, 0.1]), 0.02) for n in topo.link_names}
        want = [tuple(str(x) for x in p) for p in gold[f"pairs_{tag}"]]
        assert collision_pairs(topo, caps, cfg) == want == collision_pairs(topo, caps, cfg, world_links=()) == collision_pairs(topo, {}, cfg, boxes=caps)
        assert set(collision_set(topo, caps, cfg)) == {"capsules", "pairs", "pair_names", "margins"}


# ---- excitation: the collision block with both sets -----------------------------------------------------------------------------------------
class HostEngine:
    """candidate_capsule_distances and candidate_box_distances from the restatements: what excitation._collision_block needs of an Engine"""

    def __init__(self, topo, floating):
        self.topo, self.floating, self.n = topo, floating, topo.num_dofs

    def set_capsules(self, capsules, pairs):
        names = list(self.topo.link_names)
        self.caps = [(names.index(c.link_name), c.p0_local, c.p1_local, c.radius) for c in capsules]
        self.pairs = np.asarray(pairs).reshape(-1, 2)

    def set_boxes(self, boxes, pairs, center_in_link_axes=False):
        from box_collision_restatement import index_boxes

        self.boxes, self.box_pairs, self.cmode = index_boxes(self.topo, boxes), np.asarray(pairs).reshape(-1, 2), center_in_link_axes

    def candidate_capsule_distances(self, st, ncand, step=3, base_pos=None, device_out=None):
        import capsule_restatement as cr

        ep = cr.capsule_world(self.topo, self.caps, st["q"], self.floating, st.get("rpy"), base_pos)
        val, idx = cr.candidate_minimum(cr.capsule_distances(ep, self.caps, self.pairs)["dist"], ncand, step)
        return {"dist": val, "idx": idx}

    def candidate_box_distances(self, st, ncand, step=3, base_pos=None, device_out=None):
        R, c, h = br.box_world(self.topo, self.boxes, st["q"], self.floating, st.get("rpy"), base_pos, self.cmode)
        val, idx = br.candidate_minimum(br.pair_distances(R, c, h, self.box_pairs)[0], ncand, step)
        return {"dist": val, "idx": idx}


def kuka_mixed_set(mode, rng, placement="geometric", link_axes=False):
    """kuka: the reference's fitted capsules (lwr_6_link has none: its pairs go to the boxes in capsule mode too), a box on every link, the
    floor of world_kuka.urdf"""
    import capsule_restatement as cr
    from flobaroid_amd.collision import Box, Capsule, collision_set, world_boxes_from_urdf

    topo = load_topo("kuka_lwr4")
    gold = np.load(os.path.join(GOLDEN, "ref_capsules.npz"))
    caps = {topo.link_names[l]: Capsule(topo.link_names[l], p0, p1, r) for l, p0, p1, r in cr.fitted_capsules(gold, "kuka_lwr4", topo)}
    boxes = {topo.link_names[l]: Box(topo.link_names[l], h, c) for l, h, c, _ in synthetic_boxes(topo, rng)}
    cs = collision_set(topo, caps, {"collisionMode": mode, "worldCollisionMargin": 0.02}, boxes=boxes,
                       world_boxes=world_boxes_from_urdf(_world("kuka"), placement))
    cs["center_in_link_axes"] = link_axes
    return topo, cs


@pytest.mark.parametrize("mode,floating,link_axes", [("capsule", False, False), ("capsule", True, True), ("box", False, True), ("box", True, False)])
def test_mixed_collision_block_equals_the_sample_loop(mode, floating, link_axes):
    """g to 1e-13 (the block is computed for all samples at once, the loop one configuration at a time: NumPy's sums may be ordered
    differently), the winning samples exactly"""
    from box_collision_restatement import restate_mixed_block
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(31)
    topo, cs = kuka_mixed_set(mode, rng, link_axes=link_axes)
    assert set(cs["columns"][:, 0]) == ({0, 1} if mode == "capsule" else {1})
    C, T, n = 3, 40, topo.num_dofs
    st = random_states(topo, C * T, rng, floating, use_limits=True)
    st["q"][T:2 * T] = 0.01 * rng.standard_normal((T, n))  # (one candidate near the zero posture with the elbow turned: transitions win pairs)
    st["q"][T:2 * T, 3] += 1.95 * np.pi
    if floating:
        st["rpy"] = rng.uniform(-0.5, 0.5, (C * T, 3))
        st["base_position"] = rng.standard_normal((C * T, 3)) * 0.1 + np.array([0, 0, 0.3])
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 4, "collisionMode": mode}
    eng = HostEngine(topo, floating)
    coll = exc._collision_block(eng, st, C, config, cs)
    P = len(cs["pair_names"])
    ext = {}
    for k in ("q_min", "q_max", "dq_absmax", "tau_absmax"):
        ext[k] = rng.random((C, n))
        ext[k + "_idx"] = rng.integers(0, T, (C, n))
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    obj = exc.objectives_from_extrema(rng.random(C), np.full(C, 3), ext, limits, topo.dof_names, config, dopt_scale=1.0, collision=coll)
    lay = exc.constraint_layout(n, False, P)
    assert obj["g"].shape == (C, lay["len"])
    transitions = 0
    for c in range(C):
        sl = slice(c * T, (c + 1) * T)
        g, argmin, _ = restate_mixed_block(topo, floating, cs, st["q"][sl], config, st["rpy"][sl] if floating else None,
                                           st["base_position"][sl] if floating else None)
        assert np.abs(obj["g"][c, lay["collision"]:] - g).max() <= 1e-13
        assert all(obj["ag_cache"]["collision_argmin_idx"][c, k] == argmin.get(k, -1) for k in range(P))
        transitions += int((coll["idx"][c] < 0).sum())
    assert transitions > 0 and (obj["g"][:, lay["collision"]:] < 0).any() and (obj["g"][:, lay["collision"]:] > 0).any()
    # the gradient entry points refuse a set with box pairs
    with pytest.raises(ValueError, match="box pairs"):
        exc.candidate_collision_gradient(eng, st, C, [], 50.0, dict(config, collisionMode="capsule"), cs)
    with pytest.raises(ValueError, match="box pairs"):
        exc.candidate_gradients_from_coefficients(eng, [], T, 50.0, None, None, limits, topo.dof_names, dict(config, collisionMode="capsule"), collision=cs)
    for bad in ("convex", "full"):
        with pytest.raises(ValueError):
            exc._collision_block(eng, st, C, dict(config, collisionMode=bad), cs)


def test_box_symbols_in_header_binding_and_library():
    """added under C-ABI 104: the version stays, the binding names a library that lacks a symbol"""
    import re

    from flobaroid_amd import _lib

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    for name in ("fbr_model_set_boxes", "fbr_candidate_box_distances"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr), name
    assert lib.fbr_version() == _lib.FBR_VERSION == 104
    boxes, pairs = (int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) for k in ("FBR_MAX_BOXES", "FBR_MAX_BOX_PAIRS"))
    assert boxes >= 4 * 52 and pairs >= 16 * 1326  # a box per link of WALK-MAN and its four world boxes, every pair, with room to spare
    assert all(hasattr(_lib.Engine, a) for a in ("set_boxes", "candidate_box_distances"))
