"""The gradient entry points of excitation under ``suspended=`` on the device, both rules of ``suspended_base``: Phase C against the
yardsticks of tests/suspended_gradient_reference.py (Richardson differences of the frozen-base objective; sign(tau_swung) times the
Richardson derivative of the rest-base torque), the D-optimality gradient against the pipeline assembled on the CPU from oracle regressors
(weights at the swung base, scores at the rest or the swung base), the collision rows against central differences of the CPU
restatements' distances at the pose of ``eval_pose``, the assembly bit for bit against its parts, and the kernels' base-state arguments
against the oracle at random non-zero base states."""
import numpy as np
import pytest

import capsule_restatement as cr
import constraint_gradient_reference as cgr
import fourier_gradient_restatement as fgr
import suspended_gradient_reference as sgr
from common import load_topo, random_states
from test_suspended_gradient_host import IDS, solved

pytestmark = pytest.mark.gpu
# Ten times the error the same comparison shows with NumPy rows (tests/test_suspended_gradient_host.py), the rule and the reason of
# tests/test_gpu_candidate_gradients.py: device and NumPy round the forward differences differently, the extrema sit at the same samples.
BAR = {"held": 10.0 * sgr.MEASURED_CPU_ERROR_HELD, "identity": 10.0 * sgr.MEASURED_CPU_ERROR_IDENTITY}
RULES = ("identity", "held")
_ENGINES, _IDENTITY = {}, {}


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _engine(i):
    """the floating engine of problem i and its independent columns, made once"""
    import scipy.linalg as sla

    from flobaroid_amd._lib import Engine

    if i not in _ENGINES:
        p = solved(i)[0]
        eng = Engine(p.topo, floating=True)
        R, piv = sla.qr(eng.gram(random_states(p.topo, 2000, np.random.default_rng(1), True, use_limits=True)), pivoting=True, mode="r")
        d = np.abs(np.diag(R))
        _ENGINES[i] = (eng, np.sort(piv[: int(np.sum(d > 1e-9 * d[0]))]))
    return _ENGINES[i]


def _yardstick(i, c, rule):
    p, cands, sol = solved(i)
    J, ev, base = sol[c]
    if rule == "held":
        return J
    if (i, c) not in _IDENTITY:
        _IDENTITY[i, c] = p.identity_jacobian(p.xs[c], J, ev)
    return _IDENTITY[i, c]


def _config(p):
    return dict(p.config, collisionMode="capsule", collisionCheckStep=3, transitionDuration=3.0, transitionCollisionSamples=4)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("wf", "q_offset", "q_range", "a", "b"))


# ---- 1. Phase C ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("i", [0, 1], ids=IDS)
def test_phase_c_matches_the_yardstick_of_its_rule(i, rule):
    """3 candidates of 48 samples (the arm on LShy) and of 65 (threeLinks on its last link).  Bar: 10 x the CPU-measured error of the rule;
    printed: the largest relative error of the soft-cost gradient and of a constraint row.  The extrema's samples are the restatement's."""
    from flobaroid_amd import excitation as exc

    p, cands, sol = solved(i)
    eng, ic = _engine(i)
    n = p.n
    res = exc.candidate_gradients_from_coefficients(eng, cands, p.T, p.freq, p.x_std, ic, p.limits, p.names, _config(p), suspended=p.spec,
                                                    suspended_base=rule)
    assert not res["objectives"]["failed"].any()
    worst_soft = worst_con = 0.0
    for c in range(len(cands)):
        J, ev, base = sol[c]
        for k in cgr.IDX:
            assert np.array_equal(res["ag_cache"][k][c], ev["idx"][k]), (c, k)
        assert np.abs(res["g"][c] - ev["g"]).max() <= 1e-9 * max(np.abs(ev["g"]).max(), 1.0)
        Y = _yardstick(i, c, rule)
        kw = dict(exact=p.bounded, joint_limits=p.lim if p.bounded else None, q0=p.xs[c][1:1 + n] if p.bounded else None)
        soft = exc.gradient_to_optimizer_variables({k: v[c] for k, v in res["soft_grad"].items()}, cands[c], p.nf, **kw)
        rows = exc.constraint_gradient_to_optimizer_variables({k: v[c] for k, v in res["con_grad"].items()}, cands[c], p.nf, **kw)
        worst_soft = max(worst_soft, cgr.relative_error(soft, 10.0 * Y[0] + Y[1] + 10.0 * Y[2] + 10.0 * Y[3]))
        worst_con = max(worst_con, cgr.relative_error(rows, Y[4:]))
        assert np.abs(rows).max(axis=1).min() > 1e-3
    print(f"{IDS[i]} {rule}: relative error soft-cost gradient {worst_soft:.3e}, constraint rows {worst_con:.3e} (bar {BAR[rule]:.3e})")
    assert worst_soft <= BAR[rule] and worst_con <= BAR[rule]


# ---- 2. the D-optimality gradient -----------------------------------------------------------------------------------------------------------
def _cpu_dopt_assembly(p, cands, st, Cm, cols, k, rest_base, eps):
    """test_gpu_dopt_gradient.py's CPU pipeline with the two base states: the weight rows from the oracle's regressor at the swung states
    ``st`` (host arrays), the forward-difference scores at their rest-base view or at themselves, chained by the restatement.  Returns per
    candidate (want, bar): the bar of that test, 1e-10 max|score| / eps k per sensitivity chained through sum_t |d series|."""
    from oracle.oracle import OracleModel

    C, T, n = len(cands), p.T, p.n
    om = OracleModel(p.topo, floating=True)
    rows, P = om.rows, om.P
    Ts = (T + k - 1) // k
    S = C * Ts
    sub = {key: v.reshape(C, T, -1)[:, ::k].reshape(S, -1) for key, v in st.items() if key in ("q", "dq", "ddq", "rpy", "base_vel", "base_acc")}
    Y0 = om.regressor(sub).reshape(C, Ts * rows, P)
    W = np.zeros_like(Y0)
    W[:, :, cols] = np.einsum("grk,gkj->grj", Y0[:, :, cols], Cm)
    W = W.reshape(S, rows * P)
    at = dict(sub, **{key: np.zeros_like(sub[key]) for key in sgr.BASE_KEYS}) if rest_base else sub
    base = np.einsum("sx,sx->s", W, om.regressor(at).reshape(S, rows * P))
    sens = np.zeros((3, S, n))
    smax = np.abs(base).max()
    for kind, key in enumerate(("q", "dq", "ddq")):
        for d in range(n):
            pert = {kk: v.copy() for kk, v in at.items()}
            pert[key][:, d] += eps
            sc = np.einsum("sx,sx->s", W, om.regressor(pert).reshape(S, rows * P))
            smax = max(smax, np.abs(sc).max())
            sens[kind, :, d] = (sc - base) * (k / eps)
    A, B = np.stack([c["a"] for c in cands]), np.stack([c["b"] for c in cands])
    t = (np.arange(Ts) * k).astype(np.longdouble) / np.longdouble(p.freq)
    s_bar = 1e-10 * smax / eps * k
    out = []
    for c in range(C):
        qr = cands[c]["q_range"]
        s = [x.reshape(C, Ts, n)[c] for x in sens]
        want, _ = fgr.chain(cands[c]["wf"], qr, A[c], B[c], s[0], s[1], s[2], t)
        one = np.ones((Ts, n))
        _, dsum = fgr.chain(cands[c]["wf"], qr, A[c], B[c], one, one, one, t)
        out.append((want.astype(np.float64), s_bar * dsum.astype(np.float64)))
    return out


# (problem, engine of problem i, subsample, the two rules must differ).  The amplitude 1.5 of the arm's coefficients is chosen so that they
# do: with the CPU assembly on the restatement's base motion the largest entry-wise difference is 146 bars (subsample 1) and 139
# (subsample 2; 149 and 141 on the device's base motion); at the amplitude 0.2 of the other tests it is 17, on threeLinks between 1 and 85 for amplitudes from 0.3 to 10: that case checks the
# pipeline at n = 2 and 65 samples only.
_BIG_ARM = lambda: sgr.walkman_arm_suspended(seed=0, amps=(1.5, 1.5, 1.5))  # noqa: E731
DOPT_CASES = [(_BIG_ARM, 0, 1, True), (_BIG_ARM, 0, 2, True), (lambda: solved(1)[0], 1, 1, False)]


@pytest.mark.parametrize("make,i,k,apart_asserted", DOPT_CASES, ids=["arm-amplitude-1.5", "arm-amplitude-1.5-sub2", IDS[1]])
def test_dopt_gradient_matches_the_cpu_assembly_under_both_rules(make, i, k, apart_asserted):
    """Weights from the swung-base regressors, scores at the rest base ("identity") or the swung base ("held"); the bar of
    test_candidate_dopt_gradient_matches_cpu_assembly unchanged.  On the arm the two CPU assemblies differ by more than 100 x that bar in at
    least one entry (asserted), so a sweep at the wrong base fails.  f is candidate_dopt on the swung states times the scale."""
    from flobaroid_amd import excitation as exc

    p = make()
    cands = [p.candidate(x) for x in p.xs]
    eng, ic = _engine(i)
    C, n, nh, eps = len(cands), p.n, p.nf[0], 1e-7
    dev = exc.candidate_states(eng, cands, p.T, p.freq, suspended=p.spec)
    st = {key: _host(v) for key, v in dev.items()}
    assert np.abs(st["rpy"]).max() > 1e-3
    G = _host(eng.gram_grouped(dev, C))
    Cm, cols = exc.dopt_weight_matrices(G, ic, 1e-4, 0.5)
    wants = {}
    for rule in RULES:
        f, grad = exc.candidate_dopt_gradient_from_coefficients(eng, cands, p.T, p.freq, ic, dopt_scale=0.5, epsilon=eps, subsample=k, suspended=p.spec,
                                                                suspended_base=rule)
        assert np.array_equal(f, 0.5 * exc.candidate_dopt(eng, dev, C, ic))
        f1, grad1 = exc.candidate_dopt_gradient_from_coefficients(eng, cands, p.T, p.freq, ic, dopt_scale=0.5, epsilon=eps, subsample=k,
                                                                  max_weight_bytes=1, suspended=p.spec, suspended_base=rule)
        assert np.array_equal(f, f1) and _same(grad, grad1)  # one candidate per chunk: the same bits
        wants[rule] = _cpu_dopt_assembly(p, cands, st, Cm, cols, k, rule == "identity", eps)
        live = np.ones(1 + 2 * n + 2 * n * nh, dtype=bool) if p.bounded else np.r_[np.ones(1 + n, bool), np.zeros(n, bool), np.ones(2 * n * nh, bool)]
        worst = 0.0
        for c, (want, bar) in enumerate(wants[rule]):
            got = np.concatenate([[grad["wf"][c]], grad["q_offset"][c], grad["q_range"][c], grad["a"][c].ravel(), grad["b"][c].ravel()])
            err = np.abs(got - want)
            worst = max(worst, float((err[live] / bar[live]).max()))
            assert np.all(err[live] <= bar[live]), (rule, c, int(np.argmax(err / np.maximum(bar, 1e-300))), float(err.max()))
            assert np.linalg.norm(want) > 0
        print(f"{p.topo.name} subsample {k} {rule}: worst err / bar {worst:.3e}")
    apart = max(float((np.abs(a[0] - b[0])[live] / np.maximum(a[1], b[1])[live]).max()) for a, b in zip(wants["identity"], wants["held"]))
    print(f"{p.topo.name} subsample {k}: the two rules differ by {apart:.3e} bars")
    assert apart > 100.0 or not apart_asserted


# ---- 3. collision rows with a world geometry ----------------------------------------------------------------------------------------------
def _pose_conditions(cons, world, ref, ref0, why):
    """a world pair won on the trajectory and one won by a transition configuration at a pose other than sample 0's; for both kinds the
    row restated at the mount pose (rpy = 0, base_position = 0) is more than 100 bars from the expected row"""
    won = np.asarray(cons["g"]) < 1e10
    main = won & (np.asarray(cons["idx"]) >= 0) & world[None]
    trans = won & (np.asarray(cons["idx"]) < 0) & world[None] & (np.asarray(cons["eval_pose"]) != 0)
    assert main.any() and trans.any(), why + ": no world pair won on the trajectory / by a transition configuration: change the case"
    apart = (np.abs(ref0["grad"] - ref["grad"]) / ref["bar"]).max(-1)
    print(f"{why}: {int(main.sum())} world rows won on the trajectory, {int(trans.sum())} by a transition configuration at a pose != 0; the row at the "
          f"mount pose is {apart[main].max():.3e} / {apart[trans].max():.3e} bars away")
    assert apart[main].max() > 100.0 and apart[trans].max() > 100.0, why
    return main, trans


def test_box_rows_are_taken_at_the_pose_of_the_winning_evaluation():
    """The plain driver: collisionMode "box", the arm's boxes against three world boxes (tests/suspended_collision_cases.py), box_gradient=True.
    Every row against the central differences over analyticalGradientEpsilon of the restated box distance at rpy and base_position of
    sample ``eval_pose`` (tests/box_gradient_restatement.py, the bars of tests/test_gpu_box_gradient.py); the constraint block's winners
    are those the host finds through the restatement; the rows chained are those of candidate_collision_gradient_from_coefficients."""
    import box_gradient_restatement as bg
    import suspended_collision_cases as scc
    from flobaroid_amd import excitation as exc
    from test_box_gradient import emul_evaluate

    p, cands, sol = solved(0)
    eng, ic = _engine(0)
    C, n, T = len(cands), p.n, p.T
    config = dict(p.config, **scc.CONFIG)
    eps = config["analyticalGradientEpsilon"]
    st = exc.candidate_states(eng, cands, T, p.freq, suspended=p.spec)
    q, rpy, bp = (_host(st[k]) for k in ("q", "rpy", "base_position"))
    cs = scc.box_case(p.topo, q, rpy, bp, C)
    world = scc.world_pairs(cs)
    cons = exc._collision_block(eng, st, C, config, cs, p.spec)
    host = scc.host_constraints(p.topo, cs, {"q": q, "rpy": rpy, "base_position": bp}, C, config)
    assert np.abs(np.asarray(cons["g"]) - host["g"]).max() <= 1e-12
    for k in ("idx", "eval_sample", "eval_pose"):  # (a robot pair without a moving joint between its links may tie: the world pairs only)
        assert np.array_equal(np.asarray(cons[k])[:, world], host[k][:, world]), k
    res = exc.candidate_collision_gradient(eng, st, C, cands, p.freq, config, cs, constraints=cons, box_gradient=True, suspended=p.spec)
    smp, sc, pose = (np.asarray(cons[k]) for k in ("eval_sample", "eval_scale", "eval_pose"))
    args = (p.topo, cs["boxes"], cs["box_pairs"], True, q)
    case = {"topo": p.topo, "floating": True, "boxes": cs["boxes"], "pairs": np.asarray(cs["box_pairs"]), "q": q, "rpy": rpy, "bp": bp}
    ref = bg.evaluate(*args, rpy, bp, C, smp, sc, pose, eps, False)
    ed, _ = emul_evaluate(case, C, smp, sc, pose, eps, False)
    fin = np.isfinite(ref["dist"])
    ref = bg.with_dev(ref, float(np.abs(ed - ref["dist"])[fin].max()))
    ref0 = bg.evaluate(*args, 0.0 * rpy, 0.0 * bp, C, smp, sc, pose, eps, False)
    _pose_conditions(cons, world, ref, ref0, "box rows")
    rel = np.abs(res["grad_q"] - ref["grad"]) / ref["bar"]
    print(f"box rows: max |delta grad| / bar = {rel.max():.4f}, max |row| = {np.abs(ref['grad']).max():.3f}")
    assert np.all(rel <= 1.0) and np.all(res["grad_q"][~ref["on_path"]] == 0.0)
    assert np.all(np.abs(np.asarray(cons["g"]) - ref["dist"])[~ref["none"]] <= ref["dist_bar"][~ref["none"]])  # (the margins are zero)
    # the entry point from coefficients returns the same rows, chained
    full = exc.candidate_collision_gradient_from_coefficients(eng, cands, T, p.freq, config, cs, box_gradient=True, suspended=p.spec)
    assert np.array_equal(full["g"], np.asarray(cons["g"])) and np.array_equal(full["grad_q"], res["grad_q"]) and _same(full["grad"], res["grad"])
    assert np.abs(full["grad"]["a"][:, world]).max() > 1e-3


def test_mesh_rows_are_taken_at_the_pose_of_the_winning_evaluation():
    """The staged driver: collisionMode "convex" with fullMeshLinks, the hull set over the same boxes with one small mesh (a tetrahedron on
    the last link: tests/suspended_collision_cases.mesh_case), mesh_gradient=True.  Every row against the central differences over
    analyticalGradientEpsilon of the restated hull / mesh distance at rpy and base_position of sample ``eval_pose``
    (tests/mesh_gradient_restatement.py, the bars and the clear-verdict rule of tests/test_gpu_mesh_gradient.py)."""
    import mesh_gradient_restatement as mg
    import suspended_collision_cases as scc
    import test_mesh_gradient as tmg
    from flobaroid_amd import excitation as exc
    from test_hulls import as_tuples

    p, cands, sol = solved(0)
    eng, ic = _engine(0)
    C, T = len(cands), p.T
    st = exc.candidate_states(eng, cands, T, p.freq, suspended=p.spec)
    q, rpy, bp = (_host(st[k]) for k in ("q", "rpy", "base_position"))
    cs, config, world = scc.mesh_case(p.topo, q, rpy, bp, C)
    config = dict(p.config, **config)
    eps = config["analyticalGradientEpsilon"]
    with pytest.raises(ValueError, match="suspended"):
        exc.candidate_collision_gradient(eng, st, C, cands, p.freq, config, cs, mesh_gradient=True)
    cons = exc._collision_block(eng, st, C, config, cs, p.spec)
    res = exc.candidate_collision_gradient(eng, st, C, cands, p.freq, config, cs, constraints=cons, mesh_gradient=True, suspended=p.spec)
    smp, sc, pose = (np.asarray(cons[k]) for k in ("eval_sample", "eval_scale", "eval_pose"))
    tup, pairs = as_tuples(p.topo, cs["hulls"]), cs["hull_pairs"]
    case = {"topo": p.topo, "floating": True, "hulls": cs["hulls"], "meshes": cs["meshes"], "pairs": pairs, "q": q, "rpy": rpy, "bp": bp}
    ref = mg.evaluate(p.topo, tup, cs["meshes"], pairs, True, q, rpy, bp, C, smp, sc, pose, eps, False)
    ed, _ = tmg.emul_evaluate(case, C, smp, sc, pose, eps, False)
    live = np.isfinite(ref["dist"]) & ~ref["none"]
    ref = mg.with_dev(ref, float(np.abs(ed - ref["dist"])[live].max()))
    assert mg.clear_verdicts(ref).all(), "a stencil point of a mesh pair within 100 bars of contact: change the case"
    assert ref["meshed"].any() and (ref["meshed"] & world).any() and not ref["none"].any()
    ref0 = mg.evaluate(p.topo, tup, cs["meshes"], pairs, True, q, 0.0 * rpy, 0.0 * bp, C, smp, sc, pose, eps, False)
    _pose_conditions(cons, world, ref, ref0, "mesh rows")
    rel = np.abs(res["grad_q"] - ref["grad"]) / ref["bar"]
    print(f"mesh rows: max |delta grad| / bar = {rel.max():.4f} ({rel[:, ref['meshed']].max():.4f} over the rows of the mesh), max |row| = "
          f"{np.abs(ref['grad']).max():.3f}")
    assert np.all(rel <= 1.0) and np.all(res["grad_q"][~ref["on_path"]] == 0.0)
    assert np.all(np.abs(np.asarray(cons["g"]) - ref["dist"]) <= ref["dist_bar"])  # (the margins are zero)
    full = exc.candidate_collision_gradient_from_coefficients(eng, cands, T, p.freq, config, cs, mesh_gradient=True, suspended=p.spec)
    assert np.array_equal(full["g"], np.asarray(cons["g"])) and np.array_equal(full["grad_q"], res["grad_q"]) and _same(full["grad"], res["grad"])
    assert np.abs(full["grad"]["a"][:, world]).max() > 1e-3


def test_robot_pairs_return_the_bits_of_a_stationary_base():
    """Robot-robot box pairs with the centre offsets in link axes (in the reference's world axes the offsets do not turn with the base and
    the relative pose of two robot boxes DOES depend on it: 0.14 between the rows of the emulation): their relative pose does not depend
    on the base, and they return the bits of the same q with a stationary base.  Walked in world coordinates with the base transform
    included, the two evaluations round differently (rows 1.7e-9 apart on an MI355X, the rounding of a distance over 2 eps): the stencil of
    the rigid bodies (csrc/fbr_box_grad.h, fbr_rigidgrad_item) therefore walks a pair of two robot members with link-axes offsets from an
    identity base.  The plain driver (boxes) and the staged one (the hull set with its mesh, offsets in link axes) share that stencil;
    both are held to the bits here, rows and distances."""
    import suspended_collision_cases as scc
    from flobaroid_amd import excitation as exc

    p, cands, sol = solved(0)
    eng, ic = _engine(0)
    C, T = len(cands), p.T
    config = dict(p.config, **scc.CONFIG)
    st = exc.candidate_states(eng, cands, T, p.freq, suspended=p.spec)
    q, rpy, bp = (_host(st[k]) for k in ("q", "rpy", "base_position"))
    cs = dict(scc.box_case(p.topo, q, rpy, bp, C), center_in_link_axes=True)
    robot = ~scc.world_pairs(cs)
    cons = exc._collision_block(eng, st, C, config, cs, p.spec)
    smp, sc, pose = (np.asarray(cons[k]) for k in ("eval_sample", "eval_scale", "eval_pose"))
    eng.set_boxes(cs["boxes"], cs["box_pairs"], center_in_link_axes=True)
    kw = dict(scale=sc, pose_sample=pose, epsilon=config["analyticalGradientEpsilon"])
    swung = eng.box_distance_gradients(st, C, smp, base_pos=st["base_position"], **kw)
    still = eng.box_distance_gradients(exc.rest_base_states(st), C, smp, base_pos=0.0 * st["base_position"], **kw)
    a, b = _host(swung["grad_q"])[:, robot], _host(still["grad_q"])[:, robot]
    print(f"robot-robot rows, swung against stationary base: max |delta grad| = {np.abs(a - b).max():.3e}, max |delta dist| = "
          f"{np.abs(_host(swung['dist']) - _host(still['dist']))[:, robot].max():.3e}, max |row| = {np.abs(a).max():.3f}")
    assert np.abs(a).max() > 1e-3
    assert np.array_equal(a, b) and np.array_equal(_host(swung["dist"])[:, robot], _host(still["dist"])[:, robot])
    # a pair with a world box does depend on the base: the swung rows are not those of the mount pose
    assert np.abs(_host(swung["grad_q"])[:, ~robot] - _host(still["grad_q"])[:, ~robot]).max() > 1e-3
    # the staged driver: the hull set with one mesh
    cs, mconfig, world = scc.mesh_case(p.topo, q, rpy, bp, C)
    cs = dict(cs, offset_in_link_axes=True)
    cons = exc._collision_block(eng, st, C, dict(p.config, **mconfig), cs, p.spec)
    smp, sc, pose = (np.asarray(cons[k]) for k in ("eval_sample", "eval_scale", "eval_pose"))
    eng.set_hulls(cs["hulls"], cs["hull_pairs"], offset_in_link_axes=True, meshes=cs["meshes"])
    kw = dict(scale=sc, pose_sample=pose, epsilon=mconfig["analyticalGradientEpsilon"])
    swung = eng.mesh_distance_gradients(st, C, smp, base_pos=st["base_position"], **kw)
    still = eng.mesh_distance_gradients(exc.rest_base_states(st), C, smp, base_pos=0.0 * st["base_position"], **kw)
    a, b = _host(swung["grad_q"])[:, ~world], _host(still["grad_q"])[:, ~world]
    print(f"robot-robot rows of the hull set, swung against stationary base: max |delta grad| = {np.abs(a - b).max():.3e}, max |row| = "
          f"{np.abs(a).max():.3f}")
    assert np.abs(a).max() > 1e-3
    assert np.array_equal(a, b) and np.array_equal(_host(swung["dist"])[:, ~world], _host(still["dist"])[:, ~world])
    assert np.abs(_host(swung["grad_q"])[:, world] - _host(still["grad_q"])[:, world]).max() > 1e-3


# ---- 4. assembly ----------------------------------------------------------------------------------------------------------------------------
def _capsule_set(topo):
    caps = cr.synthetic_capsules(topo)
    pairs = cr.non_neighbour_pairs(topo, caps)
    return {"capsules": caps, "pairs": pairs, "margins": np.random.default_rng(5).uniform(0, 0.02, len(pairs))}


@pytest.mark.parametrize("rule", RULES)
def test_assembly_is_its_parts_bit_for_bit(rule):
    from flobaroid_amd import excitation as exc

    p, cands, sol = solved(0)
    eng, ic = _engine(0)
    C, n = len(cands), p.n
    cs = _capsule_set(p.topo)
    P = len(cs["pairs"])
    config = _config(p)
    args = (eng, cands, p.T, p.freq, p.x_std, ic, p.limits, p.names, config)
    res = exc.candidate_gradients_from_coefficients(*args, collision=cs, suspended=p.spec, suspended_base=rule)
    obj = exc.candidate_objectives_from_coefficients(*args, collision=cs, suspended=p.spec)
    assert np.array_equal(res["f"], obj["f"]) and np.array_equal(res["g"], obj["g"])
    lay = res["layout"]
    assert lay == exc.constraint_layout(n, True, P) and res["g"].shape == (C, lay["len"])
    scale = res["objectives"]["dopt_scale"]
    fd, gd = exc.candidate_dopt_gradient_from_coefficients(eng, cands, p.T, p.freq, ic, dopt_scale=scale, suspended=p.spec, suspended_base=rule)
    assert np.array_equal(fd, res["objectives"]["dopt"]) and _same(res["dopt_grad"], gd)
    coll = exc.candidate_collision_gradient_from_coefficients(eng, cands, p.T, p.freq, config, cs, suspended=p.spec)
    assert np.array_equal(res["g"][:, lay["collision"]:], coll["g"])
    for k, v in coll["grad"].items():
        assert np.array_equal(res["con_grad"][k][:, lay["collision"]:], v), k
        assert res["con_grad"][k].shape == (C, lay["len"]) + gd[k].shape[1:], k
        assert np.array_equal(res["obj_grad"][k], gd[k] + res["soft_grad"][k]), k
    assert np.abs(coll["grad"]["a"]).max() > 1e-3
    plain = exc.candidate_states(eng, cands, p.T, p.freq)
    info = eng.suspended_base_motion(plain, C, p.x_std, p.att_name, 1.0 / p.freq, p.damping, with_info=True)["info"]
    assert isinstance(res["suspended_info"], np.ndarray) and res["suspended_info"].shape == (C, 2)
    assert np.array_equal(res["suspended_info"], _host(info))
    again = exc.candidate_gradients_from_coefficients(*args, collision=cs, suspended=p.spec, suspended_base=rule)
    one = exc.candidate_gradients_from_coefficients(eng, cands[1:2], *args[2:], collision=cs, dopt_scale=scale, suspended=p.spec, suspended_base=rule)
    assert np.array_equal(again["f"], res["f"]) and np.array_equal(again["g"], res["g"]) and np.array_equal(again["suspended_info"], res["suspended_info"])
    assert np.array_equal(one["f"], res["f"][1:2]) and np.array_equal(one["g"], res["g"][1:2]) and np.array_equal(one["suspended_info"], res["suspended_info"][1:2])
    for part in ("obj_grad", "dopt_grad", "soft_grad", "con_grad"):
        for k in res[part]:
            assert np.array_equal(again[part][k], res[part][k]), (part, k)
            assert np.array_equal(one[part][k], res[part][k][1:2]), (part, k)


# ---- 5. nothing moves without the feature -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda: cgr.kuka_classic(friction=True), cgr.walkman_arm_floating_bounded], ids=["kuka-friction", "walkman-arm-fb-bounded"])
def test_without_suspended_every_entry_point_returns_the_bits_of_before(make):
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from test_gpu_candidate_gradients import _independent_columns

    p = make()
    eng = Engine(p.topo, floating=p.floating, friction=p.friction)
    ic = _independent_columns(eng, p.topo)
    cands = [p.candidate(x) for x in p.xs]
    C = len(cands)
    config = dict(p.config, collisionMode="capsule", collisionCheckStep=3, transitionDuration=3.0, transitionCollisionSamples=6)
    cs = _capsule_set(p.topo)
    new = {"suspended": None, "suspended_base": "identity"}
    args = (eng, cands, p.T, p.freq, p.x_std, ic, p.limits, p.names, config)
    a, b = exc.candidate_gradients_from_coefficients(*args, collision=cs), exc.candidate_gradients_from_coefficients(*args, collision=cs, **new)
    assert "suspended_info" not in a and set(a) == set(b)
    assert np.array_equal(a["f"], b["f"]) and np.array_equal(a["g"], b["g"])
    for part in ("obj_grad", "dopt_grad", "soft_grad", "con_grad"):
        assert _same(a[part], b[part]), part
    (fa, ga), (fb, gb) = (exc.candidate_dopt_gradient_from_coefficients(eng, cands, p.T, p.freq, ic, subsample=2, **kw) for kw in ({}, new))
    assert np.array_equal(fa, fb) and _same(ga, gb)
    ca = exc.candidate_collision_gradient_from_coefficients(eng, cands, p.T, p.freq, config, cs)
    cb = exc.candidate_collision_gradient_from_coefficients(eng, cands, p.T, p.freq, config, cs, suspended=None)
    st = exc.candidate_states(eng, cands, p.T, p.freq)
    cc = exc.candidate_collision_gradient(eng, st, C, cands, p.freq, config, cs, suspended=None)
    for other in (cb, cc):
        assert np.array_equal(ca["g"], other["g"]) and np.array_equal(ca["grad_q"], other["grad_q"]) and _same(ca["grad"], other["grad"])
    if eng.friction:
        import torch

        st["sign"] = torch.tanh(st["dq"] / 0.02)
    smp = a["ag_cache"]["torque_absmax_idx"]
    ja, jb = exc.candidate_torque_jacobians(eng, st, C, smp, p.x_std), exc.candidate_torque_jacobians(eng, st, C, smp, p.x_std, rest_base=False)
    assert all(np.array_equal(_host(ja[k]), _host(jb[k])) for k in ja)
    if p.floating:  # a stationary base is its own rest base: the derivatives' bits, and tau within the rounding of another kernel
        jr = exc.candidate_torque_jacobians(eng, st, C, smp, p.x_std, rest_base=True)
        assert all(np.array_equal(_host(ja[k]), _host(jr[k])) for k in ("dtau_dq", "dtau_ddq_state", "dtau_dddq"))
        assert np.abs(_host(ja["tau"]) - _host(jr["tau"])).max() <= 1e-13 * np.abs(_host(ja["tau"])).max()
    eng.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine

    p, cands, sol = solved(1)
    eng, ic = _engine(1)
    config = _config(p)
    cs = _capsule_set(p.topo)
    C = len(cands)
    args = (eng, cands, p.T, p.freq, p.x_std, ic, p.limits, p.names, config)
    st = exc.candidate_states(eng, cands, p.T, p.freq, suspended=p.spec)
    entry_points = [lambda **kw: exc.candidate_gradients_from_coefficients(*args, **kw),
                    lambda **kw: exc.candidate_dopt_gradient_from_coefficients(eng, cands, p.T, p.freq, ic, **kw)]
    for call in entry_points:
        for rule in ("Identity", "rest", None):
            with pytest.raises(ValueError, match="suspended_base"):
                call(suspended=p.spec, suspended_base=rule)
        with pytest.raises(ValueError, match="without suspended="):
            call(suspended_base="held")
        with pytest.raises(ValueError, match="unknown keys"):
            call(suspended=dict(p.spec, dampling=1.0))
    # the configuration without suspended=: all four entry points
    with pytest.raises(ValueError, match="suspended"):
        exc.candidate_gradients_from_coefficients(*args)
    with pytest.raises(ValueError, match="suspended"):
        exc.candidate_collision_gradient_from_coefficients(eng, cands, p.T, p.freq, config, cs)
    with pytest.raises(ValueError, match="suspended"):
        exc.candidate_collision_gradient(eng, st, C, cands, p.freq, config, cs)
    jac = exc.candidate_torque_jacobians(eng, st, C, np.zeros((C, p.n), dtype=np.int64), p.x_std, rest_base=True)
    with pytest.raises(ValueError, match="suspended"):
        exc.constraint_gradients_from_rows({}, jac, None, None, p.limits, p.names, config)
    # gravity-only stays refused with suspended=
    grav = dict(config, identifyGravityParamsOnly=1)
    with pytest.raises(ValueError, match="identifyGravityParamsOnly"):
        exc.candidate_gradients_from_coefficients(*args[:-1], grav, suspended=p.spec)
    with pytest.raises(ValueError, match="identifyGravityParamsOnly"):
        exc.candidate_collision_gradient_from_coefficients(eng, cands, p.T, p.freq, grav, cs, suspended=p.spec)
    with pytest.raises(ValueError, match="identifyGravityParamsOnly"):
        exc.candidate_collision_gradient(eng, st, C, cands, p.freq, grav, cs, suspended=p.spec)
    # suspended= on a fixed-base engine
    k = cgr.kuka_classic()
    fixed = Engine(k.topo)
    kc = [k.candidate(x) for x in k.xs]
    spec = {"att_link": 0, "x_std": k.x_std}
    kconf = dict(k.config, floatingBaseAttachment="suspended")
    with pytest.raises(ValueError, match="no floating base"):
        exc.candidate_gradients_from_coefficients(fixed, kc, k.T, k.freq, k.x_std, np.arange(10), k.limits, k.names, kconf, suspended=spec)
    with pytest.raises(ValueError, match="no floating base"):
        exc.candidate_dopt_gradient_from_coefficients(fixed, kc, k.T, k.freq, np.arange(10), suspended=spec)
    with pytest.raises(ValueError, match="no floating base"):
        exc.candidate_collision_gradient_from_coefficients(fixed, kc, k.T, k.freq, kconf, _capsule_set(k.topo), suspended=spec)
    fixed.close()


# ---- d. the kernels' base-state arguments -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["threeLinks", "walkman_left_arm"], ids=["n2", "n7"])
def test_sweeps_honour_a_non_zero_base_state(name):
    """fd_scores and torque_row_sweep of a floating engine at random non-zero rpy, base_vel, base_acc (65 samples: a wave and one more)
    against the oracle at the explicitly perturbed states, at the project's bars (1e-11 max|score|, 1e-11 max|tau|); the rest-base view of
    the same states gives other numbers (the base arrays are read), and those match the oracle at the zeroed base."""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from oracle.oracle import OracleModel

    topo = load_topo(name)
    n, S, eps = topo.num_dofs, 65, 1e-7
    assert n == (2 if name == "threeLinks" else 7)
    rng = np.random.default_rng(41)
    st = random_states(topo, S, rng, True, use_limits=True)
    st["rpy"] = rng.uniform(-1.0, 1.0, (S, 3))
    assert min(np.abs(st[k]).min() for k in sgr.BASE_KEYS) > 0
    eng, om = Engine(topo, floating=True), OracleModel(topo, floating=True)
    rows, P = om.rows, om.P
    W = rng.standard_normal((S * rows, P))
    x_std = topo.x_std()
    sample = rng.permutation(S)[:n].reshape(1, n).astype(np.int64)
    results = []
    for at in (st, exc.rest_base_states(st)):
        ref_sc, ref_tau = np.empty((S, 1 + 3 * n)), np.empty((1, n, 1 + 3 * n))
        Wb = W.reshape(S, rows * P)
        for col, (key, d) in enumerate([(None, 0)] + [(key, d) for key in ("q", "dq", "ddq") for d in range(n)]):
            sp = {k: v.copy() for k, v in at.items()}
            if key is not None:
                sp[key][:, d] += eps
            ref_sc[:, col] = np.einsum("sx,sx->s", Wb, om.regressor(sp).reshape(S, rows * P))
            ref_tau[0, :, col] = om.inverse_dynamics(sp, x_std)[sample[0], 6 + np.arange(n)]
        sc, sw = eng.fd_scores(at, W, eps), eng.torque_row_sweep(at, 1, sample, x_std, eps)
        err_sc, err_tau = np.abs(sc - ref_sc).max() / np.abs(ref_sc).max(), np.abs(sw - ref_tau).max() / np.abs(ref_tau).max()
        print(f"{name}: fd_scores {err_sc:.2e}, torque_row_sweep {err_tau:.2e} of the largest entry (bar 1e-11)")
        assert err_sc <= 1e-11 and err_tau <= 1e-11
        results.append((sc, sw))
    # candidate_torque_jacobians(rest_base=True) on host arrays: the derivatives of the rest-base sweep, tau of the swung states
    jac = exc.candidate_torque_jacobians(eng, st, 1, sample, x_std, eps, rest_base=True)
    swung_tau = om.inverse_dynamics(st, x_std)[sample[0], 6 + np.arange(n)]
    assert isinstance(jac["tau"], np.ndarray) and jac["tau"].shape == (1, n) and np.abs(jac["tau"][0] - swung_tau).max() <= 1e-11 * np.abs(swung_tau).max()
    assert np.array_equal(jac["dtau_dq"], (results[1][1][..., 1:1 + n] - results[1][1][..., :1]) / eps)
    assert np.array_equal(jac["dtau_dddq"], (results[1][1][..., 1 + 2 * n:] - results[1][1][..., :1]) / eps)
    assert np.abs(results[0][0] - results[1][0]).max() > 1e-3 * np.abs(results[0][0]).max()
    assert np.abs(results[0][1] - results[1][1]).max() > 1e-3 * np.abs(results[0][1]).max()
    eng.close()
