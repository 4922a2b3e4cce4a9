"""The CPU restatement of the suspended-base simulation (tests/suspended_restatement.py) checked against itself and against the
reference's own behavioural tests (tests/test_suspended.py there): the record form (b) the device kernels implement equals the direct
form (a); the record formula equals the direct Newton-Euler moment at random attachment states."""
import numpy as np
import pytest

import suspended_restatement as sr
from common import load_topo, random_topology
from np_dynamics import rpy_R


def _random_rotation(rng, S):
    from scipy.spatial.transform import Rotation

    return Rotation.random(S, random_state=int(rng.integers(1 << 30))).as_matrix()


def prismatic_tree():
    """a seeded random tree with prismatic joints and the deepest link that has one on its path: (topology, attachment link)"""
    topo = random_topology(np.random.default_rng(7), 9, p_fixed=0.2, branchiness=0.4, p_prismatic=0.4)
    best, depth = None, -1
    for l in range(topo.num_links):
        a, d, pris = l, 0, False
        while topo.parent[a] >= 0:
            pris |= topo.joint_type[a] == 2
            d += 1
            a = topo.parent[a]
        if pris and d > depth:
            best, depth = l, d
    assert best is not None
    return topo, best


def hanging_pose(topo, att, rng, trials=2000, rounds=4):
    """A joint configuration (n,) whose centre of mass lies nearly straight below the attachment origin along the attachment frame's -z:
    the swing then starts near rpy = 0, inside the reference's +-25 degree clamp.  A seeded random search on the first mass moment."""
    n = topo.num_dofs

    def tilt(q):
        z = np.zeros_like(q)
        mc = sr.sample_records(topo, att, q, z, z)[:, sr.OFF_MC:sr.OFF_MC + 3]
        return np.arctan2(np.hypot(mc[:, 0], mc[:, 1]), -mc[:, 2])

    best, sigma = np.zeros(n), 1.0
    for _ in range(rounds):
        cand = np.concatenate([best[None], best[None] + sigma * rng.standard_normal((trials, n))])
        cand = np.clip(cand, -2.5, 2.5)
        best = cand[int(np.argmin(tilt(cand)))]
        sigma *= 0.3
    return best


def smooth_states(topo, C, T, rng, freq=200.0, amp=0.4, q0=None):
    """C candidates of T samples of a one-harmonic joint motion (consistent q, dq, ddq), stacked; q0 (n,): the pose it moves about (None:
    a random one per candidate)"""
    n = topo.num_dofs
    t = np.arange(T) / freq
    A, ph, w = amp * rng.standard_normal((C, 1, n)), rng.uniform(0, 2 * np.pi, (C, 1, n)), 2 * np.pi * rng.uniform(0.3, 1.5, (C, 1, n))
    q0 = 0.3 * rng.standard_normal((C, 1, n)) if q0 is None else np.asarray(q0)[None, None, :] + 0.02 * rng.standard_normal((C, 1, n))
    arg = w * t[None, :, None] + ph
    q, dq, ddq = q0 + A * np.sin(arg), A * w * np.cos(arg), -A * w * w * np.sin(arg)
    return tuple(x.reshape(C * T, n) for x in (q, dq, ddq))


CASES = [("walkman_apriori", "crane_ft"), ("walkman_left_arm", "LShy"), ("walkman_left_arm", "LSoftHandLink"), ("walkman_left_arm", "Waist"),
         ("threeLinks", None), ("prismatic", None)]


def _case(name, att):
    if name == "prismatic":
        return prismatic_tree()
    topo = load_topo(name)
    return topo, (topo.num_links - 1 if att is None else list(topo.link_names).index(att))


@pytest.mark.parametrize("name,att", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_record_formula_equals_direct_moment(name, att):
    topo, al = _case(name, att)
    rng = np.random.default_rng(3)
    S = 6
    q, dq, ddq = ((rng.random((S, topo.num_dofs)) * 2 - 1) * x for x in (np.pi, 2.0, 5.0))
    R, om, alpha = _random_rotation(rng, S), rng.standard_normal((S, 3)), 3 * rng.standard_normal((S, 3))
    g = (0.3, -0.2, -9.81)
    direct, _ = sr.direct_moment(topo, al, q, dq, ddq, R, om, alpha, g)
    rec = sr.sample_records(topo, al, q, dq, ddq)
    got = sr.record_moment(rec, R, om, alpha, g)
    err = np.abs(got - direct).max() / np.abs(direct).max()
    print(f"{name}/{att}: record formula vs direct moment, relative {err:.2e}")
    assert err < 1e-13


def test_record_form_equals_direct_form():
    """(b) == (a): the whole simulation, left arm on a moving mid-chain link and the prismatic tree, three candidates"""
    for topo, al in (_case("walkman_left_arm", "LShy"), prismatic_tree()):
        rng = np.random.default_rng(11)
        C, T, dt = 3, 20, 1 / 200.0
        q, dq, ddq = smooth_states(topo, C, T, rng)
        a = sr.simulate_direct(topo, al, q, dq, ddq, C, dt, 500.0)
        b = sr.simulate_from_records(sr.sample_records(topo, al, q, dq, ddq), C, dt, 500.0)
        for key in ("rpy", "base_position", "base_vel", "att_state"):
            assert np.abs(a[key] - b[key]).max() < 1e-11 * max(1.0, np.abs(a[key]).max()), key
        assert np.abs(a["base_acc"] - b["base_acc"]).max() < 1e-11 * max(1.0, np.abs(a["base_vel"]).max()) / dt
        assert np.array_equal(a["info"], b["info"])


@pytest.fixture(scope="module")
def walkman():
    topo = load_topo("walkman_apriori")
    return topo, list(topo.link_names).index("crane_ft")


def test_static_equilibrium_base_stays_small(walkman):
    """the reference's test of the same name: zero joint motion, 50 samples at 200 Hz, the function's default damping; and on these inputs
    (b) equals (a) on WALK-MAN"""
    topo, att = walkman
    z = np.zeros((50, topo.num_dofs))
    b = sr.simulate_from_records(sr.sample_records(topo, att, z, z, z), 1, 1 / 200.0, 500.0)
    swing = np.abs(b["rpy"]).max()
    print(f"static: max |base_rpy| {swing:.4f}, equilibrium iterations {b['info'][0, 0]}")
    assert b["rpy"].shape == (50, 3) and b["base_vel"].shape == (50, 6) and b["base_acc"].shape == (50, 6)
    assert swing < 0.1
    assert b["info"][0, 0] < sr.EQ_MAX_ITER and b["info"][0, 1] == 0
    a = sr.simulate_direct(topo, att, z[:8], z[:8], z[:8], 1, 1 / 200.0, 500.0)
    for key in ("rpy", "base_position", "base_vel", "att_state"):
        assert np.abs(a[key] - b[key][:8]).max() < 1e-11, key
    assert a["info"][0, 0] == b["info"][0, 0]


def test_joint_motion_produces_base_swing(walkman):
    """the reference's test of the same name: a 1 Hz sinusoidal acceleration on DOF 4, 200 samples"""
    topo, att = walkman
    T, n = 200, topo.num_dofs
    t = np.arange(T) / 200.0
    q, dq, ddq = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n))
    w = 2.0 * np.pi
    ddq[:, 4] = 5.0 * np.sin(w * t)
    dq[:, 4] = -5.0 / w * np.cos(w * t) + 5.0 / w
    q[:, 4] = -5.0 / w**2 * np.sin(w * t) + 5.0 / w * t
    b = sr.simulate_from_records(sr.sample_records(topo, att, q, dq, ddq), 1, 1 / 200.0, 500.0)
    swing = np.abs(b["rpy"]).max()
    print(f"sinusoid: max |base_rpy| {swing:.4f}, equilibrium iterations {b['info'][0, 0]}")
    assert 1e-4 < swing < 1.0


def test_base_rpy_round_trip_and_short_candidates():
    """rpy_R(base_rpy) == world_R_base^T with world_R_base rebuilt from att_state and the record; base_acc is zero for T <= 2"""
    topo, al = _case("walkman_left_arm", "LSoftHandLink")
    rng = np.random.default_rng(5)
    for T in (1, 2, 3, 9):
        C = 2
        q, dq, ddq = smooth_states(topo, C, T, rng)
        rec = sr.sample_records(topo, al, q, dq, ddq)
        b = sr.simulate_from_records(rec, C, 1 / 200.0, 500.0)
        Rwb = rpy_R(b["att_state"][:, :3]) @ rec[:, sr.OFF_R:sr.OFF_R + 9].reshape(-1, 3, 3)
        assert np.abs(rpy_R(b["rpy"]) - np.swapaxes(Rwb, -1, -2)).max() < 1e-12
        if T <= 2:
            assert not b["base_acc"].any()
        else:
            assert np.abs(b["base_acc"]).max() > 0
            v = b["base_vel"].reshape(C, T, 6)
            assert np.array_equal(b["base_acc"].reshape(C, T, 6)[:, 1], (v[:, 2] - v[:, 0]) / (2 * (1 / 200.0)))
