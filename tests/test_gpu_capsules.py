"""fbr_candidate_capsule_distances / Engine.candidate_capsule_distances on the device against the NumPy restatement
(tests/capsule_restatement.py): |delta dist| <= 1e-12 max(1, largest |world coordinate|), an index may differ only between samples closer
than that; no evaluation of a committed seed sits on a branch threshold (asserted on the restatement's side before the device is looked
at, nothing is left out).  Largest difference seen on an MI355X: see DESIGN.md 8."""
import numpy as np
import pytest

import capsule_restatement as cr
from common import CONFIGS, GOLDEN, cfg_id, load_topo, random_states, random_topology

pytestmark = pytest.mark.gpu


def _engine(topo, floating, options=None):
    from flobaroid_amd._lib import Engine

    return Engine(topo, floating=floating, options=options)


def _dev(st):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in st.items()}


def _host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _caps_for(topo, name):
    if name == "kuka_lwr4":
        return cr.fitted_capsules(np.load(GOLDEN + "/ref_capsules.npz"), "kuka_lwr4", topo)
    return cr.synthetic_capsules(topo)


def _run(eng, topo, caps, pairs, st, C, step, floating, base_pos=None, device=False, why=""):
    val, idx, dist, scale = cr.device_case(topo, caps, pairs, st, C, step, floating, base_pos)
    s2 = {k: st[k] for k in ("q", "rpy") if k in st}
    if device:
        import torch

        got = eng.candidate_capsule_distances(_dev(s2), C, step, base_pos=None if base_pos is None else torch.from_numpy(base_pos).cuda())
        assert hasattr(got["dist"], "cpu")
    else:
        got = eng.candidate_capsule_distances(s2, C, step, base_pos=base_pos)
    got = _host(got)
    assert got["dist"].shape == val.shape and got["idx"].dtype == np.int64
    err = cr.assert_device_matches(got["dist"], got["idx"], val, idx, dist, C, scale, why)
    print(f"capsule case {why}: max |delta dist| = {err:.3e} (tolerance {1e-12 * scale:.3e})")
    return got


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_distances_match_the_restatement(cfg):
    name, fl = cfg[0], bool(cfg[1])
    topo = load_topo(name)
    eng = _engine(topo, fl)
    caps = _caps_for(topo, name)
    pairs = cr.non_neighbour_pairs(topo, caps)
    eng.set_capsules(caps, pairs)
    rng = np.random.default_rng(11)
    for C, T, step in ((3, 200, 3), (2, 131, 1), (5, 45, 7), (1, 300, 3)):  # T not a multiple of 64 or of step, T < 64, one candidate
        st = random_states(topo, C * T, rng, fl, use_limits=True)
        bp = rng.standard_normal((C * T, 3)) if fl else None
        if fl:
            st["rpy"] = rng.uniform(-np.pi, np.pi, (C * T, 3))
        a = _run(eng, topo, caps, pairs, st, C, step, fl, bp, device=False, why=f"{name} fb{fl} C{C} T{T} step{step} host")
        b = _run(eng, topo, caps, pairs, st, C, step, fl, bp, device=True, why=f"{name} fb{fl} C{C} T{T} step{step} device")
        assert np.array_equal(a["dist"], b["dist"]) and np.array_equal(a["idx"], b["idx"])


def test_walkman_every_link_all_pairs_and_several_launches():
    topo = load_topo("walkman_apriori")
    caps = cr.synthetic_capsules(topo)
    pairs = cr.non_neighbour_pairs(topo, caps)
    assert len(caps) == 48 and len(pairs) == 1081
    rng = np.random.default_rng(1)
    C, T = 4, 500
    st = random_states(topo, C * T, rng, True, use_limits=True)
    eng = _engine(topo, True)
    eng.set_capsules(caps, pairs)
    a = _run(eng, topo, caps, pairs, st, C, 3, True, None, device=True, why="walkman 48 capsules 1081 pairs")
    # the same in launches of two blocks each: a candidate's blocks are folded across launches, the same bits
    eng2 = _engine(topo, True, options={"chunk_samples": 128})
    eng2.set_capsules(caps, pairs)
    b = _host(eng2.candidate_capsule_distances(_dev({k: st[k] for k in ("q", "rpy")}), C, 3))
    assert np.array_equal(a["dist"], b["dist"]) and np.array_equal(a["idx"], b["idx"])


def test_many_candidates_of_a_small_robot():
    topo = load_topo("threeLinks")
    caps = cr.synthetic_capsules(topo)
    pairs = np.array([(i, j) for i in range(len(caps)) for j in range(i + 1, len(caps))], dtype=np.int32)  # (neighbours too: a small tree)
    C, T = 70001, 4
    st = random_states(topo, C * T, np.random.default_rng(3), False, use_limits=True)
    eng = _engine(topo, False)
    eng.set_capsules(caps, pairs)
    _run(eng, topo, caps, pairs, st, C, 3, False, device=True, why="70001 candidates")


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_random_trees_with_fixed_and_prismatic_joints(seed):
    rng = np.random.default_rng(seed)
    topo = random_topology(rng, int(rng.integers(5, 30)), p_fixed=0.25, branchiness=0.5, p_prismatic=0.3)
    caps = cr.synthetic_capsules(topo, radius=0.05)
    caps += [(int(rng.integers(topo.num_links)), rng.standard_normal(3) * 0.2, rng.standard_normal(3) * 0.2, 0.01) for _ in range(5)]
    pairs = cr.non_neighbour_pairs(topo, caps)
    fl = bool(seed % 2)
    C, T = 3, 150
    st = random_states(topo, C * T, rng, fl)
    eng = _engine(topo, fl)
    eng.set_capsules(caps, pairs)
    _run(eng, topo, caps, pairs, st, C, 3, fl, rng.standard_normal((C * T, 3)) if fl else None, device=True, why=f"random tree {seed}")


def test_ties_nan_overlap_spheres_and_parallel_capsules():
    topo = load_topo("kuka_lwr4")
    caps = _caps_for(topo, "kuka_lwr4")
    l2, l5 = caps[2][0], caps[5][0]
    caps = caps + [(l5, np.array([0.0, 0.0, 0.05]), np.array([0.0, 0.0, 0.05]), 0.04),       # a sphere
                   (l2, np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.2]), 0.03),         # two exactly parallel capsules on one link
                   (l2, np.array([0.1, 0.0, 0.05]), np.array([0.1, 0.0, 0.15]), 0.03),
                   (l2, np.array([0.01, 0.0, 0.0]), np.array([0.01, 0.0, 0.2]), 0.03),       # ... and one that overlaps the first
                   (caps[0][0], np.zeros(3), np.zeros(3), 0.01)]                            # a sphere on the base
    n0 = len(caps) - 5
    pairs = np.concatenate([cr.non_neighbour_pairs(topo, caps[:n0]), [[0, n0], [n0, n0 + 4], [n0 + 1, n0 + 2], [n0 + 1, n0 + 3], [1, n0]]]).astype(np.int32)
    eng = _engine(topo, False)
    eng.set_capsules(caps, pairs)
    rng = np.random.default_rng(4)
    T = 96
    one = random_states(topo, T, rng, False, use_limits=True)["q"]
    q = np.concatenate([one, one, one[:40], one[:40], one[:24]])  # candidate 0: two identical periods; candidate 1: twice 40 samples, then others
    C = 2
    # ties: the first of the two identical samples wins, at every step that keeps the periods aligned
    got = _run(eng, topo, caps, pairs, {"q": q[:2 * T]}, 1, 1, False, device=True, why="ties")
    assert got["idx"].max() < T
    got = _run(eng, topo, caps, pairs, {"q": q[:2 * T]}, 1, 3, False, device=True, why="ties step 3")
    assert got["idx"].max() < T
    # overlap: a negative distance, the same at every sample (both capsules ride on one link)
    k = len(pairs) - 2
    assert np.all(got["dist"][:, k] < 0)
    # exactly parallel capsules: compared like every other pair (a e - b^2 at rounding level, far from the threshold)
    # NaN: a sample with NaN q is skipped; a candidate of NaN only returns 1e10 / -1
    qn = q.copy()
    val0, idx0, _, _ = cr.device_case(topo, caps, pairs, {"q": q}, C, 1, False)
    for c in range(C):
        for kk in range(len(pairs)):
            if idx0[c, kk] >= 0:
                qn[c * (len(q) // C) + idx0[c, kk]] = np.nan  # (knock out a winning sample: another one has to win)
                break
    got = _run(eng, topo, caps, pairs, {"q": qn}, C, 1, False, device=True, why="NaN samples")
    qa = np.full_like(q, np.nan)
    got = _host(eng.candidate_capsule_distances({"q": qa}, C, 1))
    assert np.all(got["dist"] == 1e10) and np.all(got["idx"] == -1)


def test_same_bits_every_run_and_a_replaced_set_is_used():
    topo = load_topo("walkman_apriori")
    caps = cr.synthetic_capsules(topo)
    pairs = cr.non_neighbour_pairs(topo, caps)
    rng = np.random.default_rng(6)
    C, T = 8, 333
    st = random_states(topo, C * T, rng, True, use_limits=True)
    dev = _dev({k: st[k] for k in ("q", "rpy")})
    eng = _engine(topo, True)
    eng.set_capsules(caps, pairs)
    a = _host(eng.candidate_capsule_distances(dev, C, 3))
    b = _host(eng.candidate_capsule_distances(dev, C, 3))
    assert a["dist"].tobytes() == b["dist"].tobytes() and a["idx"].tobytes() == b["idx"].tobytes()
    caps2 = [(l, p0, p1, r + 0.01) for l, p0, p1, r in caps[:20]]
    pairs2 = cr.non_neighbour_pairs(topo, caps2)[::-1].copy()  # (another order as well: not sorted by the first capsule)
    eng.set_capsules(caps2, pairs2)
    _run(eng, topo, caps2, pairs2, st, C, 3, True, device=True, why="replaced set")


def test_invalid_arguments_are_refused_and_the_handle_survives():
    from flobaroid_amd._lib import FbrError

    topo = load_topo("kuka_lwr4")
    caps = _caps_for(topo, "kuka_lwr4")
    pairs = cr.non_neighbour_pairs(topo, caps)
    eng = _engine(topo, False)
    st = random_states(topo, 60, np.random.default_rng(0), False, use_limits=True)
    with pytest.raises(FbrError, match="code -1"):  # no capsule set
        eng.candidate_capsule_distances(st, 2, 3)
    bad = [([(99, np.zeros(3), np.zeros(3), 0.1)], np.zeros((0, 2))),             # link out of range
           (caps, [[0, len(caps)]]), (caps, [[1, 1]]),                                 # pair index out of range, a capsule with itself
           ([(0, np.zeros(3), np.ones(3), -0.1)] + caps[1:], pairs),                   # negative radius
           ([(0, np.zeros(3), np.ones(3), np.inf)] + caps[1:], pairs),
           ([(0, np.array([0, np.nan, 0]), np.ones(3), 0.1)] + caps[1:], pairs),       # non-finite end point
           ([(0, np.zeros(3), np.ones(3), 0.1)] * 4097, pairs)]                        # more than FBR_MAX_CAPSULES
    eng.set_capsules(caps, pairs)
    for c, p in bad:
        with pytest.raises(FbrError, match="code -1"):
            eng.set_capsules(c, p)
    assert eng.num_capsule_pairs == len(pairs)  # (the set in place before a refused call stays: used again below)
    _run(eng, topo, caps, pairs, st, 2, 3, False, device=False, why="set kept after refused replacements")
    for C, step, S in ((0, 3, 60), (2, 0, 60), (7, 3, 60)):  # ncand < 1, step < 1, not a multiple
        with pytest.raises(FbrError, match="code -1"):
            eng.candidate_capsule_distances({"q": st["q"][:S]}, C, step)
    eng.set_capsules(caps, np.zeros((0, 2)))
    with pytest.raises(FbrError, match="code -1"):  # npairs = 0
        eng.candidate_capsule_distances(st, 2, 3)
    eng.set_capsules([], [])
    with pytest.raises(FbrError, match="code -1"):  # cleared
        eng.candidate_capsule_distances(st, 2, 3)
    eng.set_capsules(caps, pairs)
    _run(eng, topo, caps, pairs, st, 2, 3, False, device=False, why="after refused calls")
    tau = eng.inverse_dynamics(st, topo.x_std())
    assert np.isfinite(tau).all()


def test_objectives_from_coefficients_with_collision_end_to_end():
    """candidate_objectives_from_coefficients(collision=...) against the host restatement of the collision block on the host copy of the
    device-generated states; without the argument the result is what it is with collision=None"""
    from collision_restatement import restate_collision_block
    from flobaroid_amd import excitation as exc
    from flobaroid_amd.collision import Capsule, collision_set

    topo = load_topo("kuka_lwr4")
    eng = _engine(topo, False)
    caps = {topo.link_names[l]: Capsule(topo.link_names[l], p0, p1, r) for l, p0, p1, r in _caps_for(topo, "kuka_lwr4")}
    rng = np.random.default_rng(12)
    cs = collision_set(topo, caps, {"collisionMaxKinematicDistance": 0})
    cs["margins"] = rng.uniform(0, 0.02, len(cs["pair_names"]))
    n, C, T, freq = topo.num_dofs, 5, 150, 50.0
    cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.3 for _ in range(n)], [rng.standard_normal(2) * 0.3 for _ in range(n)],
                                      rng.uniform(-0.2, 0.2, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 6, "collisionMode": "capsule"}
    import scipy.linalg as sla

    cols = np.sort(sla.qr(eng.gram(random_states(topo, 2000, np.random.default_rng(1), False, use_limits=True)), pivoting=True, mode="r")[1][:43])
    base = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, dopt_scale=1.0)
    full = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, dopt_scale=1.0,
                                                      collision=cs)
    P = len(cs["pair_names"])
    assert full["g"].shape == (C, 5 * n + P) and np.array_equal(full["g"][:, :5 * n], base["g"]) and np.array_equal(full["f"], base["f"])
    st = exc.candidate_states(eng, cands, T, freq, device=True)
    q = st["q"].cpu().numpy()
    names = list(topo.link_names)
    caps_i = [(names.index(c.link_name), c.p0_local, c.p1_local, c.radius) for c in cs["capsules"]]
    ep = cr.capsule_world(topo, caps_i, q)
    assert int(cr.capsule_distances(ep, caps_i, cs["pairs"])["near"].sum()) == 0
    tol = 1e-12 * max(1.0, cr.world_scale(ep))
    for c in range(C):
        g, argmin = restate_collision_block(topo, False, caps_i, cs["pairs"], cs["margins"], q[c * T:(c + 1) * T], config)
        assert np.abs(full["g"][c, 5 * n:] - g).max() <= tol
        got = full["ag_cache"]["collision_argmin_idx"][c]
        assert all(got[k] == argmin.get(k, -1) for k in range(P))
