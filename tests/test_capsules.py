"""Capsule collision distances off the GPU: the NumPy restatement (tests/capsule_restatement.py) is pinned on the reference's recorded
outputs, the HIP-free text of csrc/fbr_capsule.h (segment routine, positions-only walk; g++, tests/emul/capsule_emul.cpp) is held against
both, the host module flobaroid_amd/collision.py reproduces the reference's fitted capsules and pair lists, and
excitation.objectives_from_extrema(collision=...) equals a sample-by-sample restatement of the reference's collision block."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import capsule_restatement as cr
from collision_restatement import restate_collision_block
from common import GOLDEN, ROOT, load_topo, random_states, random_topology

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "capsule_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libcapsule_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lp = ctypes.POINTER(ctypes.c_long)
_lib = None


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC] + [os.path.join(_CSRC, h) for h in ("fbr_capsule.h", "fbr_math.h", "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def emul_eval(topo, floating, capsules, pairs, q, rpy=None, base_pos=None):
    """(ep (S, ncaps, 6), dist (S, P), st (S, P, 2)) from the library's own lane walk and segment routine on the CPU"""
    c = lambda a, t=np.float64: np.ascontiguousarray(a, dtype=t)  # noqa: E731
    parent, dof = c(topo.parent, np.int32), c(topo.dof_index, np.int32)
    jt = c(topo.joint_type, np.int32)
    rR, rp, ax = c(topo.rest_R).reshape(-1), c(topo.rest_p).reshape(-1), c(topo.axis).reshape(-1)
    link = c([k[0] for k in capsules], np.int32)
    seg = c([np.concatenate([k[1], k[2]]) for k in capsules]).reshape(-1)
    rad = c([k[3] for k in capsules])
    pr = c(pairs, np.int32).reshape(-1)
    q = c(q)
    S, P = q.shape[0], pr.size // 2
    rpy = None if rpy is None else c(rpy)
    bp = None if base_pos is None else c(base_pos)
    ep, dist, st = np.zeros((S, len(capsules), 6)), np.zeros((S, P)), np.zeros((S, P, 2))
    rc = emul().cap_eval(topo.num_links, topo.num_dofs, parent.ctypes.data_as(_ip), dof.ctypes.data_as(_ip), _d(rR), _d(rp), _d(ax),
                         jt.ctypes.data_as(_ip), int(floating), len(capsules), link.ctypes.data_as(_ip), _d(seg), _d(rad), P, pr.ctypes.data_as(_ip),
                         ctypes.c_long(S), _d(q), _d(rpy), _d(bp), _d(ep), _d(dist), _d(st))
    assert rc == 0
    return ep, dist, st


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "ref_capsules.npz"))


def _gold_world(z):
    f = lambda R, p, x: np.einsum("sij,sj->si", R, x) + p  # noqa: E731
    return (f(z["cd_Ra"], z["cd_pa"], z["cd_p0a"]), f(z["cd_Ra"], z["cd_pa"], z["cd_p1a"]), f(z["cd_Rb"], z["cd_pb"], z["cd_p0b"]),
            f(z["cd_Rb"], z["cd_pb"], z["cd_p1b"]))


def test_restatement_equals_the_reference_on_every_branch(gold):
    """distances to 1e-15 absolute.  s and t to 1e-15 times their conditioning (capsule_restatement.parameter_condition): with the very
    world end points the reference returned as input, s still differs by 1.7e-15 in one record (a 4.7 cm segment, |r| = 1: -c / a with
    a = 2.2e-3) because the reference's dot products are BLAS calls with another rounding than a left-to-right sum -- measured: at most 0.31
    of eps times that conditioning, the bar leaves a factor 14."""
    a0, a1, b0, b1 = _gold_world(gold)
    assert np.abs(np.concatenate([a0, a1, b0, b1], axis=1) - gold["cd_world"]).max() <= 1e-15
    a0, a1, b0, b1 = (np.ascontiguousarray(gold["cd_world"][:, 3 * k:3 * k + 3]) for k in range(4))
    out = cr.segment_distance(a0, a1, b0, b1)
    # every branch of the segment routine occurs in the records
    assert set(out["branch"].tolist()) == {cr.BOTH_POINTS * 3, cr.A_POINT * 3, cr.B_POINT * 3} | {c * 3 + t for c in (cr.GENERAL, cr.PARALLEL)
                                                                                                   for t in (cr.T_INSIDE, cr.T_BELOW, cr.T_ABOVE)}
    assert not out["near"].any()
    dist = out["dist"] - gold["cd_ra"] - gold["cd_rb"]
    assert np.abs(dist - gold["cd_dist"]).max() <= 1e-15
    tol = 1e-15 * cr.parameter_condition(a0, a1, b0, b1)
    assert np.all(np.abs(out["s"] - gold["cd_s"]) <= tol) and np.all(np.abs(out["t"] - gold["cd_t"]) <= tol)
    exact = cr.parameter_condition(a0, a1, b0, b1) == 1.0  # (degenerate and well conditioned records: the plain 1e-15)
    assert exact.any() and np.abs(out["s"] - gold["cd_s"])[exact].max() <= 1e-15
    assert (gold["cd_dist"] < 0).any()


def test_library_segment_routine_equals_the_reference_on_every_branch(gold):
    w = np.ascontiguousarray(gold["cd_world"])
    out = np.zeros(3)
    cond = cr.parameter_condition(*(w[:, 3 * k:3 * k + 3] for k in range(4)))  # (s, t: see the test above)
    for i in range(w.shape[0]):
        a0, a1, b0, b1 = (np.ascontiguousarray(w[i, 3 * k:3 * k + 3]) for k in range(4))
        emul().cap_segment(_d(a0), _d(a1), _d(b0), _d(b1), _d(out))
        assert abs(out[0] - gold["cd_ra"][i] - gold["cd_rb"][i] - gold["cd_dist"][i]) <= 1e-15, i
        assert abs(out[1] - gold["cd_s"][i]) <= 1e-15 * cond[i] and abs(out[2] - gold["cd_t"][i]) <= 1e-15 * cond[i], i


def _check_walk(topo, floating, caps, pairs, st, base_pos):
    ep = cr.capsule_world(topo, caps, st["q"], floating, st.get("rpy"), base_pos)
    want = cr.capsule_distances(ep, caps, pairs)
    assert int(want["near"].sum()) == 0
    ep2, dist, stp = emul_eval(topo, floating, caps, pairs, st["q"], st.get("rpy") if floating else None, base_pos if floating else None)
    tol = 1e-12 * max(1.0, cr.world_scale(ep))
    assert np.abs(ep2 - ep).max() <= tol
    assert np.abs(dist - want["dist"]).max() <= tol
    return np.abs(dist - want["dist"]).max()


def test_library_walk_kuka_fitted_capsules(gold):
    topo = load_topo("kuka_lwr4")
    caps = cr.fitted_capsules(gold, "kuka_lwr4", topo)
    assert len(caps) == 7  # (of the 8 fitted: one sits on a massless link that the topology keeps as a frame only)
    pairs = cr.non_neighbour_pairs(topo, caps)
    st = random_states(topo, 2000, np.random.default_rng(1), False, use_limits=True)
    _check_walk(topo, False, caps, pairs, st, None)
    # spheres have a squared length of exactly zero in the library's walk: both end points come from one expression
    sph = [(c[0], c[1], c[1].copy(), c[3]) for c in caps]
    ep, _, _ = emul_eval(topo, False, sph, pairs, st["q"][:50])
    assert np.array_equal(ep[..., :3], ep[..., 3:])


def test_library_walk_walkman_floating_every_link(gold):
    topo = load_topo("walkman_apriori")
    caps = cr.synthetic_capsules(topo)
    pairs = cr.non_neighbour_pairs(topo, caps)
    assert len(caps) == 48 and len(pairs) == 1081
    rng = np.random.default_rng(1)
    st = random_states(topo, 300, rng, True, use_limits=True)
    st["rpy"] = rng.uniform(-np.pi, np.pi, (300, 3))
    _check_walk(topo, True, caps, pairs, st, rng.standard_normal((300, 3)))
    _check_walk(topo, True, caps, pairs, st, None)


@pytest.mark.parametrize("seed", [3, 4, 5, 6])
def test_library_walk_random_trees_with_fixed_and_prismatic_joints(seed):
    rng = np.random.default_rng(seed)
    topo = random_topology(rng, int(rng.integers(5, 30)), p_fixed=0.25, branchiness=0.5, p_prismatic=0.3)
    caps = cr.synthetic_capsules(topo, radius=0.05)
    caps += [(int(rng.integers(topo.num_links)), rng.standard_normal(3) * 0.2, rng.standard_normal(3) * 0.2, 0.01) for _ in range(5)]  # several per link
    pairs = cr.non_neighbour_pairs(topo, caps)
    fl = bool(seed % 2)
    st = random_states(topo, 200, rng, fl)
    _check_walk(topo, fl, caps, pairs, st, rng.standard_normal((200, 3)) if fl else None)


def test_candidate_minimum_rules():
    rng = np.random.default_rng(9)
    T, P = 40, 6
    d = rng.standard_normal((T, P))
    d[:, 1] = np.nan                  # never wins: 1e10, -1
    d[5, 2] = d[17, 2] = d[:, 2].min() - 1.0  # a tie: the first sample
    d[0, 3] = np.nan                  # a NaN first sample does not stick
    d[:, 4] = 2e10                    # nothing below the initial 1e10
    for step in (1, 3, 7):
        val, idx = cr.candidate_minimum(d, 1, step)
        v2, i2 = np.zeros(P), np.zeros(P, dtype=np.int64)
        emul().cap_minimum(ctypes.c_long(T), ctypes.c_long(step), P, _d(np.ascontiguousarray(d)), _d(v2), i2.ctypes.data_as(_lp))
        assert np.array_equal(val[0], v2) and np.array_equal(idx[0], i2)
        assert val[0, 1] == 1e10 and idx[0, 1] == -1 and val[0, 4] == 1e10 and idx[0, 4] == -1
        # against the plain loop
        for k in range(P):
            b, ib = 1e10, -1
            for t in range(0, T, step):
                if d[t, k] < b:
                    b, ib = d[t, k], t
            assert (val[0, k], idx[0, k]) == (b, ib)
    assert cr.candidate_minimum(d, 1, 1)[1][0, 2] == 5


# ---- flobaroid_amd/collision.py ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["kuka_lwr4", "threeLinks"])
def test_fit_capsules_equals_the_reference(gold, robot):
    from flobaroid_amd.collision import fit_capsules_from_urdf
    import xml.etree.ElementTree as ET

    urdf = os.path.join(GOLDEN, "urdf", robot + ".urdf")
    names = [l.attrib["name"] for l in ET.parse(urdf).findall("link")]
    for scale, tag in ((1.0, ""), (0.8, "_s08")):
        caps, mesh_only = fit_capsules_from_urdf(urdf, names, radius_scale=scale)
        assert list(caps) == [str(n) for n in gold[f"fit_{robot}{tag}_links"]]
        assert np.array_equal(np.array([c.p0_local for c in caps.values()]), gold[f"fit_{robot}{tag}_p0"])
        assert np.array_equal(np.array([c.p1_local for c in caps.values()]), gold[f"fit_{robot}{tag}_p1"])
        assert np.array_equal(np.array([c.radius for c in caps.values()]), gold[f"fit_{robot}{tag}_radius"])
        assert mesh_only == (["lwr_6_link"] if robot == "kuka_lwr4" else [])  # (a mesh: no capsule in the reference's record either)
        assert not set(mesh_only) & set(caps)


def test_fit_capsules_reports_mesh_only_links():
    from flobaroid_amd.collision import fit_capsules_from_urdf
    import xml.etree.ElementTree as ET

    urdf = os.path.join(GOLDEN, "urdf", "walkman_apriori.urdf")
    names = [l.attrib["name"] for l in ET.parse(urdf).findall("link")]
    caps, mesh_only = fit_capsules_from_urdf(urdf, names)
    with_coll = [l.attrib["name"] for l in ET.parse(urdf).findall("link") if l.findall("collision")]
    assert sorted(list(caps) + mesh_only) == sorted(with_coll) and not set(caps) & set(mesh_only)


@pytest.mark.parametrize("tag", ["kuka_all", "kuka_ignore", "walkman_dist5", "walkman_all"])
def test_collision_pairs_equal_the_reference(gold, tag):
    from flobaroid_amd.collision import Capsule, collision_pairs, collision_set

    topo = load_topo(str(gold[f"pairs_{tag}_robot"]))
    cfg = json.loads(str(gold[f"pairs_{tag}_config"]))
    caps = {n: Capsule(n, np.zeros(3), np.array([0, 0, 0.1]), 0.02) for n in topo.link_names}
    got = collision_pairs(topo, caps, cfg)
    assert got == [tuple(str(x) for x in p) for p in gold[f"pairs_{tag}"]]
    cs = collision_set(topo, caps, cfg)
    assert [(cs["capsules"][a].link_name, cs["capsules"][b].link_name) for a, b in cs["pairs"]] == got
    # a link without a capsule is not checked
    first = got[0][0]
    fewer = collision_pairs(topo, {k: v for k, v in caps.items() if k != first}, cfg)
    assert fewer == [p for p in got if first not in p]


# ---- excitation: the collision block ------------------------------------------------------------------------------------------------
class HostEngine:
    """candidate_capsule_distances from the restatement: what excitation.candidate_collision_constraints needs of an Engine"""

    def __init__(self, topo, floating):
        self.topo, self.floating, self.n = topo, floating, topo.num_dofs

    def set_capsules(self, capsules, pairs):
        names = list(self.topo.link_names)
        self.caps = [(names.index(c.link_name), c.p0_local, c.p1_local, c.radius) for c in capsules]
        self.pairs = np.asarray(pairs).reshape(-1, 2)

    def candidate_capsule_distances(self, st, ncand, step=3, base_pos=None, device_out=None):
        ep = cr.capsule_world(self.topo, self.caps, st["q"], self.floating, st.get("rpy"), base_pos)
        val, idx = cr.candidate_minimum(cr.capsule_distances(ep, self.caps, self.pairs)["dist"], ncand, step)
        return {"dist": val, "idx": idx}


def _kuka_collision(gold, rng, margins=True):
    from flobaroid_amd.collision import Capsule, collision_set

    topo = load_topo("kuka_lwr4")
    caps = {topo.link_names[l]: Capsule(topo.link_names[l], p0, p1, r) for l, p0, p1, r in cr.fitted_capsules(gold, "kuka_lwr4", topo)}
    cs = collision_set(topo, caps, {})
    if margins:
        cs["margins"] = rng.uniform(0.0, 0.05, len(cs["pair_names"]))
    return topo, cs


@pytest.mark.parametrize("floating,transition", [(False, 3.0), (True, 3.0), (False, 0.0)])
def test_collision_block_equals_the_sample_loop(gold, floating, transition):
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(21)
    topo, cs = _kuka_collision(gold, rng)
    C, T = 3, 50
    st = random_states(topo, C * T, rng, floating, use_limits=True)
    # one candidate stays near the zero posture with its elbow turned by almost a full revolution: the ramps from / to zero fold the arm
    # on their way, so that transition configurations win pairs there
    st["q"][T:2 * T] = 0.01 * rng.standard_normal((T, topo.num_dofs))
    st["q"][T:2 * T, 3] += 1.95 * np.pi
    if floating:
        st["rpy"] = rng.uniform(-0.5, 0.5, (C * T, 3))
        st["base_position"] = rng.standard_normal((C * T, 3)) * 0.1
    config = {"collisionCheckStep": 3, "transitionDuration": transition, "transitionCollisionSamples": 5, "collisionMode": "capsule"}
    eng = HostEngine(topo, floating)
    eng.set_capsules(cs["capsules"], cs["pairs"])
    got = exc.candidate_collision_constraints(eng, st, C, config, margins=cs["margins"])
    won_by_transition = 0
    for c in range(C):
        sl = slice(c * T, (c + 1) * T)
        g, argmin = restate_collision_block(topo, floating, eng.caps, eng.pairs, cs["margins"], st["q"][sl], config,
                                            st["rpy"][sl] if floating else None, st["base_position"][sl] if floating else None)
        assert np.array_equal(got["g"][c], g)
        for k in range(len(g)):
            assert got["argmin"][c, k] == argmin.get(k, -1)
        won_by_transition += int((got["idx"][c] < 0).sum())
    assert (won_by_transition > 0) == (transition > 0)


def test_transition_indices_are_the_reference_numbering(gold):
    """the negative index of a winning transition configuration counts the reference's configurations, repeated base poses dropped"""
    from flobaroid_amd import excitation as exc
    from collision_restatement import transition_configs

    rng = np.random.default_rng(5)
    topo, cs = _kuka_collision(gold, rng, margins=False)
    C, T = 2, 30
    st = random_states(topo, C * T, rng, True, use_limits=True)
    st["rpy"] = rng.uniform(-0.5, 0.5, (C * T, 3))
    st["rpy"][0] = 3.0  # the extreme swing of candidate 0 is a sample the even spacing already holds: six distinct poses there
    config = {"transitionDuration": 3.0, "transitionCollisionSamples": 3}
    eng = HostEngine(topo, True)
    eng.set_capsules(cs["capsules"], cs["pairs"])
    got = exc.candidate_collision_constraints(eng, st, C, config)
    for c in range(C):
        sl = slice(c * T, (c + 1) * T)
        tc = transition_configs(st["q"][sl], st["rpy"][sl], None, config)
        assert len(tc) == 2 * 3 * (6 if c == 0 else 7)
        for k in np.nonzero(got["idx"][c] < 0)[0]:
            i, q, r, _ = tc[-got["idx"][c, k] - 1]
            assert i == got["idx"][c, k]
            d = cr.capsule_distances(cr.capsule_world(topo, eng.caps, q[None], True, r[None]), eng.caps, eng.pairs)["dist"][0, k]
            assert d == got["g"][c, k]


def test_objectives_with_and_without_collision(gold):
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(2)
    topo, cs = _kuka_collision(gold, rng)
    C, T, n = 2, 20, topo.num_dofs
    st = random_states(topo, C * T, rng, False, use_limits=True)
    ext = {}
    for k in ("q_min", "q_max", "dq_absmax", "tau_absmax"):
        ext[k] = rng.random((C, n))
        ext[k + "_idx"] = rng.integers(0, T, (C, n))
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    config = {"minVelocityConstraint": False}
    base = exc.objectives_from_extrema(rng.random(C), np.full(C, 3), ext, limits, topo.dof_names, config, dopt_scale=1.0)
    again = exc.objectives_from_extrema(np.array(base["dopt"]), np.full(C, 3), ext, limits, topo.dof_names, config, dopt_scale=1.0, collision=None)
    assert set(base) == set(again) and set(base["ag_cache"]) == set(again["ag_cache"]) and "collision_argmin_idx" not in base["ag_cache"]
    assert base["g"].shape == (C, 5 * n) and np.array_equal(base["g"], again["g"])
    assert "collision" not in exc.constraint_layout(n, False)
    eng = HostEngine(topo, False)
    eng.set_capsules(cs["capsules"], cs["pairs"])
    coll = exc.candidate_collision_constraints(eng, st, C, config, margins=cs["margins"])
    with_c = exc.objectives_from_extrema(np.array(base["dopt"]), np.full(C, 3), ext, limits, topo.dof_names, config, dopt_scale=1.0, collision=coll)
    P = len(cs["pair_names"])
    lay = exc.constraint_layout(n, False, P)
    assert lay["collision"] == 5 * n and lay["len"] == 5 * n + P and with_c["g"].shape == (C, lay["len"])
    assert np.array_equal(with_c["g"][:, :5 * n], base["g"]) and np.array_equal(with_c["g"][:, 5 * n:], coll["g"])
    assert np.array_equal(with_c["ag_cache"]["collision_argmin_idx"], coll["argmin"])
    for k in ("f", "f1", "f2", "f3", "f4", "dopt"):
        assert np.array_equal(with_c[k], again[k])
