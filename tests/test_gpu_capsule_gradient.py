"""fbr_capsule_distance_gradients / fbr_fourier_position_chain and excitation.candidate_collision_gradient on the device against the NumPy
restatement (tests/capsule_gradient_restatement.py): per item |delta grad| <= 1e-12 max(1, world scale) parameter_condition, the distance to
1e-12 max(1, world scale), joints off a pair's path exactly 0.0; no evaluation of a committed seed sits on a branch threshold (asserted on
the restatement's side)."""
import numpy as np
import pytest

import capsule_gradient_restatement as cg
import capsule_restatement as cr
from common import load_topo, random_states, random_topology
from test_capsule_gradient import shifted_capsules

pytestmark = pytest.mark.gpu
T = 7


def _engine(topo, floating):
    from flobaroid_amd._lib import Engine

    return Engine(topo, floating=floating)


def _cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _robot(name):
    rng = np.random.default_rng({"threeLinks": 1, "kuka_lwr4": 2, "walkman_left_arm": 3, "random": 4}[name])
    fl = name == "walkman_left_arm"
    topo = random_topology(rng, 17, p_fixed=0.25, branchiness=0.5, p_prismatic=0.3) if name == "random" else load_topo(name)
    caps = shifted_capsules(topo, rng)
    pairs = cr.non_neighbour_pairs(topo, caps)
    if len(pairs) == 0:
        pairs = np.array([(i, j) for i in range(len(caps)) for j in range(i + 1, len(caps))], dtype=np.int32)
    return topo, fl, caps, pairs, rng


def _compare(got, ref, why):
    assert not ref["near"][ref["dist"] < cr.NONE].any(), "an evaluation of this seed lies on a branch threshold: change the seed"
    none = ref["dist"] == cr.NONE
    assert np.all(got["dist"][none] == cr.NONE) and np.all(got["grad_q"][none] == 0.0), why
    errd = np.abs(got["dist"] - ref["dist"])[~none].max() if (~none).any() else 0.0
    tol = cg.gradient_tolerance(ref)
    rel = (np.abs(got["grad_q"] - ref["grad"]).max(axis=2) / tol)[~none].max() if (~none).any() else 0.0
    print(f"{why}: max |delta dist| = {errd:.3e} (tolerance {1e-12 * ref['scale']:.1e}), max |delta grad| / tolerance = {rel:.4f}")
    assert errd <= 1e-12 * ref["scale"], why
    assert rel <= 1.0, why
    assert np.all(got["grad_q"][~ref["on_path"]] == 0.0), why


@pytest.mark.parametrize("name", ["threeLinks", "kuka_lwr4", "walkman_left_arm", "random"])
def test_device_matches_the_restatement(name):
    """C = 1 (one lane), 3 (a ragged wave), 64 (an exact wave), 65 and 130 (a wave never spans two pairs), P from 1 to every non-neighbour
    pair; samples 0, T - 1, interior and -1 mixed; scale NULL (host arrays) and random in (0, 1] (device tensors); pose_sample != sample"""
    topo, fl, caps, all_pairs, rng = _robot(name)
    eng = _engine(topo, fl)
    for C, P in ((1, 1), (3, min(2, len(all_pairs))), (64, len(all_pairs)), (65, len(all_pairs)), (130, min(3, len(all_pairs)))):
        pairs = all_pairs[rng.choice(len(all_pairs), P, replace=False)] if P < len(all_pairs) else all_pairs
        pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]
        eng.set_capsules(caps, pairs)
        st = random_states(topo, C * T, rng, False, use_limits=name != "random")
        q = st["q"]
        rpy = rng.uniform(-np.pi, np.pi, (C * T, 3)) if fl else None
        bp = rng.standard_normal((C * T, 3)) if fl else None
        sample = rng.choice([0, T - 1, 1, 2, 3, 4, 5, -1], size=(C, P), p=[0.2, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1]).astype(np.int64)
        sample[0, 0] = T - 1
        pose = ((sample + 1 + rng.integers(0, T - 1, (C, P))) % T).astype(np.int64)
        pose[sample < 0] = -1
        states = {"q": q} if rpy is None else {"q": q, "rpy": rpy}
        # scale NULL, host arrays
        got = eng.capsule_distance_gradients(states, C, sample, pose_sample=pose, base_pos=bp)
        assert isinstance(got["dist"], np.ndarray) and got["grad_q"].shape == (C, P, topo.num_dofs)
        _compare(got, cg.evaluate(topo, caps, pairs, fl, q, rpy, bp, C, sample, None, pose), f"{name} C{C} P{P} scale NULL")
        # random scale, device tensors
        scale = rng.uniform(0.05, 1.0, (C, P))
        dstates = {k: _cuda(v) for k, v in states.items()}
        gd = eng.capsule_distance_gradients(dstates, C, _cuda(sample), scale=_cuda(scale), pose_sample=_cuda(pose), base_pos=_cuda(bp))
        assert hasattr(gd["dist"], "cpu")
        _compare(_host(gd), cg.evaluate(topo, caps, pairs, fl, q, rpy, bp, C, sample, scale, pose), f"{name} C{C} P{P} random scale")
        # main-trajectory items: the distance fbr_candidate_capsule_distances returns with step = 1 on one-sample candidates
        smp = np.repeat(rng.integers(0, T, (C, 1)), P, axis=1).astype(np.int64)
        one = eng.capsule_distance_gradients(states, C, smp, base_pos=bp)
        rows = np.arange(C) * T + smp[:, 0]
        st1 = {"q": q[rows]} if rpy is None else {"q": q[rows], "rpy": rpy[rows]}
        main = eng.candidate_capsule_distances(st1, C, 1, base_pos=None if bp is None else bp[rows])
        ep = cr.capsule_world(topo, caps, q[rows], fl, None if rpy is None else rpy[rows], None if bp is None else bp[rows])
        assert np.all(main["idx"] == 0) and np.abs(one["dist"] - main["dist"]).max() <= 1e-12 * max(1.0, cr.world_scale(ep))


def test_chain_on_the_device_matches_the_restatement():
    """classic and bounded, host and device inputs, rows with sample -1, a random scale and NULL: against the long-double restatement to
    1e-12 |scale| sum_d |grad_q[d]| max(1, q_range) per row.  Every |dq_d/dp| here (|a|, |b| ~ 0.4, three harmonics, t <= 0.6 s, wf >= 0.8) is
    below 5 and is formed with about twenty roundings of doubles: 5 * 20 * 1.1e-16 ~ 1e-14 per unit of |scale grad_q|, two decades below
    the bar; a wrong expression is off by the size of the entries, 0.1 .. 1."""
    topo = load_topo("kuka_lwr4")
    eng = _engine(topo, False)
    rng = np.random.default_rng(3)
    n, nh, C, R, freq = topo.num_dofs, 3, 3, 37, 10.0
    A, B = rng.standard_normal((C, n, nh)) * 0.4, rng.standard_normal((C, n, nh)) * 0.4
    wf = rng.uniform(0.8, 1.4, C)
    sample = rng.integers(-1, T, (C, R)).astype(np.int64)
    sample[0, :3] = [0, T - 1, -1]
    g = rng.standard_normal((C, R, n)) * (rng.random((C, R, n)) < 0.5)  # (exact zeros, as the joints off a pair's path)
    for qr in (None, rng.uniform(0.5, 1.5, (C, n))):
        for scale, device in ((None, False), (rng.uniform(0.05, 1.0, (C, R)), True)):
            if device:
                got = eng.fourier_position_chain(wf, A, B, _cuda(sample), _cuda(g), freq, scale=_cuda(scale), q_range=qr)
                assert hasattr(got, "cpu")
                got = got.cpu().numpy()
            else:
                got = eng.fourier_position_chain(wf, A, B, sample, g, freq, scale=scale, q_range=qr)
            for c in range(C):
                want = cg.position_chain(wf[c], None if qr is None else qr[c], A[c], B[c], sample[c], None if scale is None else scale[c], g[c], freq,
                                         dtype=np.longdouble).astype(np.float64)
                sc = np.ones(R) if scale is None else scale[c]
                bound = 1e-12 * sc * np.abs(g[c]).sum(axis=1) * (1.0 if qr is None else max(1.0, qr[c].max()))
                assert np.all(np.abs(got[c] - want) <= bound[:, None]), (qr is None, device, c, np.abs(got[c] - want).max())
                assert np.abs(want).max() > 0.1
                assert np.all(got[c][sample[c] < 0] == 0.0)


def test_corner_rules():
    """coincident closest points: zero row, unchanged distance; spheres and parallel capsules follow the restatement; a NaN row of q gives
    NaN in that item only; sample -1 gives 1e10 and zeros; two runs give the same bits"""
    from np_dynamics import world_kinematics

    topo = load_topo("kuka_lwr4")
    rng = np.random.default_rng(5)
    caps = shifted_capsules(topo, rng)
    l2, l3, l6 = caps[2][0], caps[3][0], caps[6][0]
    C = 4
    q = random_states(topo, C * T, rng, False, use_limits=True)["q"]
    z = np.zeros((1, 3))
    kin = world_kinematics(topo, q[:1], 0 * q[:1], 0 * q[:1], np.eye(3)[None], z, z, z, z)
    w = kin["R"][l6, 0] @ np.array([0.0, 0.0, 0.1]) + kin["p"][l6, 0]
    local3 = kin["R"][l3, 0].T @ (w - kin["p"][l3, 0])
    caps = caps + [(l6, np.array([0.0, 0.0, 0.1]), np.array([0.0, 0.0, 0.1]), 0.02), (l3, local3, local3.copy(), 0.03),  # coincide at sample 0 of candidate 0
                   (l2, np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.2]), 0.03),                                   # exactly parallel, one link
                   (l2, np.array([0.1, 0.0, 0.05]), np.array([0.1, 0.0, 0.15]), 0.03),
                   (l6, np.array([0.0, 0.05, 0.0]), np.array([0.0, 0.05, 0.2]), 0.02)]                                  # parallel to nothing in general
    n0 = len(caps) - 5
    pairs = np.array([[0, 6], [1, 5], [2, n0 + 4], [n0, n0 + 1], [n0 + 2, n0 + 3], [n0 + 2, n0 + 4]], dtype=np.int32)
    P = len(pairs)
    eng = _engine(topo, False)
    eng.set_capsules(caps, pairs)
    sample = rng.integers(0, T, (C, P)).astype(np.int64)
    sample[0, :] = 0
    sample[1, 2] = -1
    sample[3, :] = 4
    got = eng.capsule_distance_gradients({"q": q}, C, sample)
    ref = cg.evaluate(topo, caps, pairs, False, q, None, None, C, sample)
    _compare(got, ref, "corner rules")
    assert abs(got["dist"][0, 3] + 0.05) <= 1e-12 and np.all(got["grad_q"][0, 3] == 0.0)  # coincident: -r_a - r_b, a zero row
    assert np.all(got["grad_q"][:, 4] == 0.0) and np.all(np.isfinite(got["dist"][:, 4]))   # two capsules of one link: nothing moves them apart
    assert got["dist"][1, 2] == 1e10 and np.all(got["grad_q"][1, 2] == 0.0)
    again = eng.capsule_distance_gradients({"q": q}, C, sample)
    assert got["dist"].tobytes() == again["dist"].tobytes() and got["grad_q"].tobytes() == again["grad_q"].tobytes()
    qn = q.copy()
    qn[3 * T + 4] = np.nan  # the row every item of candidate 3 evaluates
    gn = eng.capsule_distance_gradients({"q": qn}, C, sample)
    assert np.array_equal(gn["dist"][:3], got["dist"][:3]) and np.array_equal(gn["grad_q"][:3], got["grad_q"][:3])
    moved = np.array([caps[a][0] != caps[b][0] for a, b in pairs])  # (a pair on one link reads no joint below the base ... its pose is NaN all the same)
    assert np.all(np.isnan(gn["dist"][3])) and np.all(np.isnan(gn["grad_q"][3][ref["on_path"][3]]))
    assert np.all(gn["grad_q"][3][~ref["on_path"][3]] == 0.0) and moved.any()


def test_invalid_arguments_are_refused_and_the_handle_survives():
    from flobaroid_amd._lib import FbrError

    topo = load_topo("kuka_lwr4")
    caps = shifted_capsules(topo, np.random.default_rng(0))
    pairs = cr.non_neighbour_pairs(topo, caps)
    P = len(pairs)
    eng = _engine(topo, False)
    q = random_states(topo, 2 * T, np.random.default_rng(0), False, use_limits=True)["q"]
    ok = np.zeros((2, P), dtype=np.int64)
    with pytest.raises(FbrError, match="code -1"):  # no capsule set
        eng.capsule_distance_gradients({"q": q}, 2, np.zeros((2, 0), dtype=np.int64))
    eng.set_capsules(caps, np.zeros((0, 2)))
    with pytest.raises(FbrError, match="code -1"):  # a set without pairs
        eng.capsule_distance_gradients({"q": q}, 2, np.zeros((2, 0), dtype=np.int64))
    eng.set_capsules(caps, pairs)
    with pytest.raises(FbrError, match="code -1"):  # ncand < 1
        eng.capsule_distance_gradients({"q": q}, 0, np.zeros((1, P), dtype=np.int64))
    with pytest.raises(FbrError, match="code -1"):  # not a multiple
        eng.capsule_distance_gradients({"q": q[:13]}, 2, ok)
    for bad_sample, bad_pose in ((T, None), (-2, None), (10**12, None), (0, T), (0, -5)):
        s = ok.copy()
        s[1, P - 1] = bad_sample
        pose = None
        if bad_pose is not None:
            pose = ok.copy()
            pose[0, 0] = bad_pose
        with pytest.raises(FbrError, match="code -1"):
            eng.capsule_distance_gradients({"q": q}, 2, s, pose_sample=pose)
    got = eng.capsule_distance_gradients({"q": q}, 2, ok)
    _compare(got, cg.evaluate(topo, caps, pairs, False, q, None, None, 2, ok), "after refused calls")
    with pytest.raises(FbrError, match="code -1"):
        eng.fourier_position_chain(np.ones(1), np.zeros((1, topo.num_dofs, 2)), np.zeros((1, topo.num_dofs, 2)), np.zeros((1, 1), dtype=np.int64),
                                   np.zeros((1, 1, topo.num_dofs)), 0.0)  # freq must be positive
    assert np.isfinite(eng.inverse_dynamics(random_states(topo, 5, np.random.default_rng(1), False, use_limits=True), topo.x_std())).all()


SEEDS = {False: 4, True: 4}  # chosen so that a transition configuration wins at least one pair of the perturbed candidate (asserted)


@pytest.mark.parametrize("bounded", [False, True], ids=["classic", "bounded"])
def test_collision_gradient_end_to_end(bounded):
    """candidate_collision_gradient_from_coefficients on kuka_lwr4, 3 candidates, T = 60, collisionCheckStep 3, transitions on: every
    optimiser variable of one candidate moved by +-1e-6, the distance re-evaluated on the device at the same fixed evaluation points
    (capsule_distance_gradients' dist), the central difference against the constraint_gradient_to_optimizer_variables row at 1e-8 (the bar
    of the restatement's own finite-difference test)."""
    from flobaroid_amd import excitation as exc

    topo = load_topo("kuka_lwr4")
    eng = _engine(topo, False)
    rng = np.random.default_rng(SEEDS[bounded])
    caps = shifted_capsules(topo, rng)
    pairs = cr.non_neighbour_pairs(topo, caps)
    n, C, Tn, freq = topo.num_dofs, 3, 60, 20.0
    nf = [2] * n
    lim = [(topo.limits[j]["lower"], topo.limits[j]["upper"]) for j in topo.dof_names]

    def make(x):
        a = [x[1 + n + 2 * j:1 + n + 2 * j + 2] for j in range(n)]
        b = [x[1 + 3 * n + 2 * j:1 + 3 * n + 2 * j + 2] for j in range(n)]
        return exc.fourier_coefficients(a, b, x[1:1 + n], nf, wf=float(x[0]), joint_limits=lim if bounded else None)

    xs = [np.concatenate([[rng.uniform(0.8, 1.2)], rng.uniform(-0.2, 0.2, n), rng.standard_normal(4 * n) * 0.5]) for _ in range(C)]
    cands = [make(x) for x in xs]
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 6, "collisionMode": "capsule"}
    cs = {"capsules": caps, "pairs": pairs}
    res = exc.candidate_collision_gradient_from_coefficients(eng, cands, Tn, freq, config, cs)
    P = len(pairs)
    assert res["g"].shape == (C, P) and res["grad"]["a"].shape == (C, P, n, 2) and res["grad_q"].shape == (C, P, n)
    st = exc.candidate_states(eng, cands, Tn, freq, device=True)
    cons = exc.candidate_collision_constraints(eng, st, C, config)
    assert np.array_equal(cons["g"], res["g"])
    main = cons["idx"] >= 0
    assert np.array_equal(cons["eval_sample"][main], cons["idx"][main]) and np.all(cons["eval_scale"][main] == 1.0)
    c = int(np.argmax(((cons["idx"] < 0) & (cons["g"] < 1e10)).sum(axis=1)))
    trans = (cons["idx"][c] < 0) & (cons["g"][c] < 1e10)
    assert trans.any(), "no transition configuration wins a pair of any candidate: choose another seed"
    assert np.all(np.isin(cons["eval_sample"][c][trans], (0, Tn - 1))) and np.all((cons["eval_scale"][c][trans] > 0) & (cons["eval_scale"][c][trans] < 1))
    rows = exc.constraint_gradient_to_optimizer_variables({k: v[c] for k, v in res["grad"].items()}, cands[c], nf, exact=bounded,
                                                          joint_limits=lim if bounded else None, q0=xs[c][1:1 + n] if bounded else None)
    assert rows.shape == (P, xs[c].size)
    ev = {k: cons[k][c:c + 1] for k in ("eval_sample", "eval_scale", "eval_pose")}

    def dist(x):
        s1 = exc.candidate_states(eng, [make(x)], Tn, freq, device=True)
        return eng.capsule_distance_gradients(s1, 1, ev["eval_sample"], scale=ev["eval_scale"], pose_sample=ev["eval_pose"])["dist"].cpu().numpy()[0]

    base = dist(xs[c])
    assert np.abs(base - res["g"][c]).max() <= 1e-12
    fd = np.zeros_like(rows)
    for v in range(xs[c].size):
        xp, xm = xs[c].copy(), xs[c].copy()
        xp[v] += 1e-6
        xm[v] -= 1e-6
        fd[:, v] = (dist(xp) - dist(xm)) / 2e-6
    err = np.abs(fd - rows)
    print(f"end to end, bounded={bounded}: max |row - FD| = {err.max():.3e} (transition rows: {err[trans].max():.3e}), max |row| = {np.abs(rows).max():.3f}, "
          f"{int(trans.sum())} of {P} pairs won by a transition configuration")
    assert err.max() <= 1e-8
    assert np.abs(rows[trans]).max() > 1e-3
