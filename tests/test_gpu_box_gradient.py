"""fbr_box_distance_gradients / Engine.box_distance_gradients and excitation.candidate_collision_gradient(box_gradient=True) on the device
against the NumPy restatement (tests/box_gradient_restatement.py: whole re-walks at q +- eps e_d for every joint): per entry |delta grad| <=
bar, bar = (b+ + b-) / (2 eps) with b+- = max(10 dev, 32 EPS pair_scale) the bar of the box distances at the two stencil points (dev: the g++
emulation's largest deviation from the restatement over the case's distances); the distance within its bar; entries the stencil never
touches exactly 0.0.

Largest |delta grad| / bar measured on an MI355X over the 16 cases (four robots, both centre modes, both steps): 0.075 (kuka_lwr4, centres in
link axes, eps = 1e-7); per robot threeLinks 0.035, kuka_lwr4 0.075, walkman_left_arm 0.043, random tree 0.027 (every case prints its own)."""
import numpy as np
import pytest

import box_gradient_restatement as bg
import capsule_gradient_restatement as cg
from common import load_topo, random_states
from test_box_gradient import ROBOTS, T, emul_evaluate, item_arrays, make_case

pytestmark = pytest.mark.gpu
_CASES, _ENGINES = {}, {}


def _case(robot):
    if robot not in _CASES:
        _CASES[robot] = make_case(robot, C=65)
    return _CASES[robot]


def _engine(robot):
    from flobaroid_amd._lib import Engine

    if robot not in _ENGINES:
        case = _case(robot)
        _ENGINES[robot] = Engine(case["topo"], floating=case["floating"])
    return _ENGINES[robot]


def _cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _sub(case, C):
    """the first C candidates of the case"""
    fl = case["floating"]
    return dict(case, C=C, q=case["q"][:C * T], rpy=case["rpy"][:C * T] if fl else None, bp=case["bp"][:C * T] if fl else None)


def _reference(sub, pairs, sample, scale, pose, eps, mode):
    C = sub["C"]
    ref = bg.evaluate(sub["topo"], sub["boxes"], pairs, sub["floating"], sub["q"], sub["rpy"], sub["bp"], C, sample, scale, pose, eps, mode)
    ed, _ = emul_evaluate(sub, C, sample, scale, pose, eps, mode, pairs)
    fin = np.isfinite(ref["dist"])
    assert np.array_equal(fin, np.isfinite(ed))
    return bg.with_dev(ref, float(np.abs(ed - ref["dist"])[fin].max()))


def _compare(got, ref, why):
    """the largest |delta grad| / bar, after the assertions"""
    none = ref["none"]
    assert got["dist"].shape == ref["dist"].shape and got["grad_q"].shape == ref["grad"].shape, why
    assert np.all(got["dist"][none] == bg.NONE) and np.all(got["grad_q"][none] == 0.0), why
    errd = (np.abs(got["dist"] - ref["dist"]) / ref["dist_bar"])[~none]
    rel = np.abs(got["grad_q"] - ref["grad"]) / ref["bar"]
    print(f"{why}: max |delta dist| / bar = {errd.max() if errd.size else 0.0:.3f}, max |delta grad| / bar = {rel.max():.4f}")
    assert np.all(errd <= 1.0), why
    assert np.all(rel <= 1.0), why
    assert np.all(got["grad_q"][~ref["on_path"]] == 0.0), why
    return float(rel.max())


def _states(sub, device):
    st = {"q": sub["q"]} if not sub["floating"] else {"q": sub["q"], "rpy": sub["rpy"]}
    return ({k: _cuda(v) for k, v in st.items()}, _cuda(sub["bp"])) if device else (st, sub["bp"])


@pytest.mark.parametrize("eps", [1e-7, 1e-4])
@pytest.mark.parametrize("mode", [False, True], ids=["world-axes", "link-axes"])
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_device_matches_the_restatement(robot, mode, eps):
    """C = 1 (one lane), 3 (a ragged wave), 64 (an exact wave), 65 (a wave never spans two pairs), P from 1 to every pair of the case; samples
    0, T - 1, interior and -1 mixed; scale NULL (host arrays) and random in (0, 1] (device tensors); pose_sample != sample; then one-sample
    candidates against fbr_candidate_box_distances with step = 1"""
    case, eng = _case(robot), _engine(robot)
    rng = np.random.default_rng(21)
    allp = case["pairs"]
    worst = 0.0
    for C, P in ((1, 1), (1, len(allp)), (3, len(allp)), (64, 2), (65, 3)):
        pairs = allp[np.sort(rng.choice(len(allp), P, replace=False))] if P < len(allp) else allp
        sub = _sub(case, C)
        eng.set_boxes(case["boxes"], pairs, center_in_link_axes=mode)
        sample, scale, pose = item_arrays(sub, rng, C, P, True)
        st, bp = _states(sub, False)
        got = eng.box_distance_gradients(st, C, sample, pose_sample=pose, base_pos=bp, epsilon=eps)
        assert isinstance(got["dist"], np.ndarray) and got["grad_q"].shape == (C, P, case["topo"].num_dofs)
        worst = max(worst, _compare(got, _reference(sub, pairs, sample, None, pose, eps, mode), f"{robot} mode {int(mode)} eps {eps:g} C{C} P{P} scale NULL"))
        dst, dbp = _states(sub, True)
        gd = eng.box_distance_gradients(dst, C, _cuda(sample), scale=_cuda(scale), pose_sample=_cuda(pose), base_pos=dbp, epsilon=eps)
        assert hasattr(gd["dist"], "cpu")
        ref = _reference(sub, pairs, sample, scale, pose, eps, mode)
        worst = max(worst, _compare(_host(gd), ref, f"{robot} mode {int(mode)} eps {eps:g} C{C} P{P} random scale"))
        # main-trajectory items: the distance fbr_candidate_box_distances returns with step = 1 on one-sample candidates
        smp = np.repeat(rng.integers(0, T, (C, 1)), P, axis=1).astype(np.int64)
        one = eng.box_distance_gradients(st, C, smp, base_pos=bp, epsilon=eps)
        rows = np.arange(C) * T + smp[:, 0]
        st1 = {k: v[rows] for k, v in st.items()}
        main = eng.candidate_box_distances(st1, C, 1, base_pos=None if bp is None else bp[rows])
        r1 = _reference(sub, pairs, smp, None, None, eps, mode)
        assert np.all(main["idx"] == 0) and np.all(np.abs(one["dist"] - main["dist"]) <= r1["dist_bar"])
    print(f"{robot} mode {int(mode)} eps {eps:g}: largest |delta grad| / bar = {worst:.4f}")


def test_corner_rules():
    """two boxes on one link (centres in link axes): zero rows and a finite distance; sample -1: 1e10 and a zero row; two runs give the same
    bytes; a NaN row of q poisons that candidate's items only, and its untouched entries are still exactly 0"""
    case, eng = _case("kuka_lwr4"), _engine("kuka_lwr4")
    topo, boxes = case["topo"], list(case["boxes"])
    boxes.append((boxes[4][0], np.array([0.05, 0.04, 0.03]), np.array([0.3, 0.0, 0.1]), None))
    pairs = np.concatenate([case["pairs"][:6], [[4, len(boxes) - 1]]]).astype(np.int32)
    C, P, eps = 4, len(pairs), 1e-7
    sub = dict(_sub(case, C), boxes=boxes)
    rng = np.random.default_rng(9)
    sample = rng.integers(0, T, (C, P)).astype(np.int64)
    sample[1, 2] = -1
    sample[3, :] = 4
    eng.set_boxes(boxes, pairs, center_in_link_axes=True)
    got = eng.box_distance_gradients({"q": sub["q"]}, C, sample, epsilon=eps)
    ref = _reference(sub, pairs, sample, None, None, eps, True)
    _compare(got, ref, "corner rules")
    assert np.all(got["grad_q"][:, P - 1] == 0.0) and np.all(np.isfinite(got["dist"][:, P - 1])) and not ref["on_path"][:, P - 1].any()
    assert got["dist"][1, 2] == 1e10 and np.all(got["grad_q"][1, 2] == 0.0)
    again = eng.box_distance_gradients({"q": sub["q"]}, C, sample, epsilon=eps)
    assert got["dist"].tobytes() == again["dist"].tobytes() and got["grad_q"].tobytes() == again["grad_q"].tobytes()
    qn = sub["q"].copy()
    qn[3 * T + 4] = np.nan  # the row every item of candidate 3 evaluates
    gn = eng.box_distance_gradients({"q": qn}, C, sample, epsilon=eps)
    assert np.array_equal(gn["dist"][:3], got["dist"][:3]) and np.array_equal(gn["grad_q"][:3], got["grad_q"][:3])
    assert np.all(np.isnan(gn["dist"][3])) and np.all(np.isnan(gn["grad_q"][3][ref["on_path"][3]]))
    assert np.all(gn["grad_q"][3][~ref["on_path"][3]] == 0.0) and (~ref["on_path"][3]).any()


def test_invalid_arguments_are_refused_and_the_sets_do_not_touch_each_other():
    from flobaroid_amd._lib import FbrError
    from test_capsule_gradient import shifted_capsules
    import capsule_restatement as cr

    case = _case("kuka_lwr4")
    topo, boxes, pairs = case["topo"], case["boxes"], case["pairs"]
    from flobaroid_amd._lib import Engine

    eng = Engine(topo, floating=False)
    P = len(pairs)
    sub = _sub(case, 2)
    st = {"q": sub["q"]}
    ok = np.zeros((2, P), dtype=np.int64)
    caps = shifted_capsules(topo, np.random.default_rng(0))
    cpairs = cr.non_neighbour_pairs(topo, caps)
    eng.set_capsules(caps, cpairs)
    csmp = np.ones((2, len(cpairs)), dtype=np.int64)
    before = eng.capsule_distance_gradients(st, 2, csmp)
    with pytest.raises(FbrError, match="code -1"):  # no box set
        eng.box_distance_gradients(st, 2, np.zeros((2, 0), dtype=np.int64))
    eng.set_boxes(boxes, np.zeros((0, 2)))
    with pytest.raises(FbrError, match="code -1"):  # a set without pairs
        eng.box_distance_gradients(st, 2, np.zeros((2, 0), dtype=np.int64))
    eng.set_boxes(boxes, pairs, center_in_link_axes=True)
    with pytest.raises(FbrError, match="code -1"):  # ncand < 1
        eng.box_distance_gradients(st, 0, np.zeros((1, P), dtype=np.int64))
    with pytest.raises(FbrError, match="code -1"):  # not a multiple
        eng.box_distance_gradients({"q": sub["q"][:13]}, 2, ok)
    for bad_sample, bad_pose in ((T, None), (-2, None), (10**12, None), (0, T), (0, -5)):
        s = ok.copy()
        s[1, P - 1] = bad_sample
        pose = None
        if bad_pose is not None:
            pose = ok.copy()
            pose[0, 0] = bad_pose
        with pytest.raises(FbrError, match="code -1"):
            eng.box_distance_gradients(st, 2, s, pose_sample=pose)
    for bad in (0.0, -1e-7, float("nan"), float("inf")):
        with pytest.raises(FbrError, match="code -1"):
            eng.box_distance_gradients(st, 2, ok, epsilon=bad)
    got = eng.box_distance_gradients(st, 2, ok, epsilon=1e-7)
    _compare(got, _reference(sub, pairs, ok, None, None, 1e-7, True), "after refused calls")
    assert np.isfinite(eng.inverse_dynamics(random_states(topo, 5, np.random.default_rng(1), False, use_limits=True), topo.x_std())).all()
    after = eng.capsule_distance_gradients(st, 2, csmp)
    assert before["dist"].tobytes() == after["dist"].tobytes() and before["grad_q"].tobytes() == after["grad_q"].tobytes()
    eng.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
SEEDS = {"capsule": 4, "box": 4}  # chosen so that a transition configuration wins a box pair (asserted) and at most 10 % of the rows sit on a kink
FD_BAR = 6e-8


def _restated_rows(topo, cs, cons, q, cands, c, freq, eps, sel):
    """rows (len(sel), E) of candidate c's box pairs ``sel`` (merged positions): the restated grad_q at the evaluation points chained in long
    double, and the bound per row and parameter"""
    from box_collision_restatement import index_boxes

    boxes = index_boxes(topo, cs["boxes"])
    cols = np.asarray(cs["columns"])
    bp = np.asarray(cs["box_pairs"]).reshape(-1, 2)[cols[sel, 1]]
    C = len(cands)
    pick = lambda k: np.ascontiguousarray(np.asarray(cons[k])[:, sel])  # noqa: E731
    mode = bool(cs.get("center_in_link_axes", False))
    ref = bg.evaluate(topo, boxes, bp, False, q, None, None, C, pick("eval_sample"), pick("eval_scale"), pick("eval_pose"), eps, mode)
    sub = {"topo": topo, "floating": False, "boxes": boxes, "pairs": bp, "q": q, "rpy": None, "bp": None}
    ed, _ = emul_evaluate(sub, C, pick("eval_sample"), pick("eval_scale"), pick("eval_pose"), eps, mode, bp)
    fin = np.isfinite(ref["dist"])
    ref = bg.with_dev(ref, float(np.abs(ed - ref["dist"])[fin].max()))
    cand = cands[c]
    smp, sc = pick("eval_sample")[c], pick("eval_scale")[c]
    want = cg.position_chain(cand["wf"], cand["q_range"], cand["a"], cand["b"], smp, sc, ref["grad"][c], freq, dtype=np.longdouble).astype(np.float64)
    # |d row| <= |scale| sum_d bar[d] |dq_d/dp|: the chain of the bars is the chain restatement on them (its entries are >= 0 for >= 0 rows
    # only column by column, so the absolute Jacobian is taken joint by joint)
    n = topo.num_dofs
    bound = np.zeros_like(want)
    for d in range(n):
        e = np.zeros((len(sel), n))
        e[:, d] = ref["bar"][c][:, d]
        bound += np.abs(cg.position_chain(cand["wf"], cand["q_range"], cand["a"], cand["b"], smp, sc, e, freq))
    qr = 1.0 if cand["q_range"] is None else max(1.0, float(np.max(cand["q_range"])))
    bound += (1e-12 * np.abs(sc) * np.abs(ref["grad"][c]).sum(axis=1) * qr)[:, None]
    return ref, want, bound


@pytest.mark.parametrize("mode", ["capsule", "box"])
def test_collision_gradient_end_to_end(mode):
    """kuka_mixed_set, C = 3, T = 60, collisionCheckStep 3, transitions on.  g equals the objective's collision block; the capsule columns
    equal the capsule-only set through the existing path byte for byte; the box rows equal the restated chain within the chained bars; then
    every optimiser variable of one candidate is moved by +-1e-6, the box distances re-evaluated on the device at the fixed evaluation points
    and the central difference held against the constraint_gradient_to_optimizer_variables rows.

    FD_BAR: the same experiment with the NumPy restatement alone (its distances differenced over +-1e-6 in the variables against its own
    chained rows at eps = 1e-7) gives 2.6e-9 (capsule mode, 13 box rows) and 5.8e-9 (box mode, 29 rows) on the committed seed, every row
    keeping the sign of its SAT gap: 5.8e-9 x 10, rounded up, 6e-8.  The rows that do not keep it are left out, 10 % of the box rows at most
    (asserted).  Measured on an MI355X: 4.1e-9 (capsule mode) and 6.1e-9 (box mode), no row left out; the box rows within 0.031 and 0.046 of
    the chained bars of the restated chain."""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from test_boxes import kuka_mixed_set
    from test_gpu_box_objectives import _cols

    rng = np.random.default_rng(SEEDS[mode])
    topo, cs = kuka_mixed_set(mode, rng, link_axes=mode == "box")
    eng = Engine(topo, floating=False)
    n, C, Tn, freq, eps = topo.num_dofs, 3, 60, 20.0, 1e-7
    nf = [2] * n

    def make(x):
        a = [x[1 + n + 2 * j:1 + n + 2 * j + 2] for j in range(n)]
        b = [x[1 + 3 * n + 2 * j:1 + 3 * n + 2 * j + 2] for j in range(n)]
        return exc.fourier_coefficients(a, b, x[1:1 + n], nf, wf=float(x[0]))

    xs = [np.concatenate([[rng.uniform(0.8, 1.2)], rng.uniform(-0.2, 0.2, n), rng.standard_normal(4 * n) * 0.5]) for _ in range(C)]
    cands = [make(x) for x in xs]
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 5, "collisionMode": mode,
              "analyticalGradientEpsilon": eps}
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    cols = np.asarray(cs["columns"])
    P = len(cols)
    res = exc.candidate_collision_gradient_from_coefficients(eng, cands, Tn, freq, config, cs, box_gradient=True)
    assert res["g"].shape == (C, P) and res["grad"]["a"].shape == (C, P, n, 2) and res["grad_q"].shape == (C, P, n)
    icols = _cols(eng, topo, False)
    obj = exc.candidate_objectives_from_coefficients(eng, cands, Tn, freq, topo.x_std(), icols, limits, topo.dof_names, config, dopt_scale=1.0, collision=cs)
    lay = exc.constraint_layout(n, False, P)
    assert np.array_equal(res["g"], obj["g"][:, lay["collision"]:])
    st = exc.candidate_states(eng, cands, Tn, freq, device=True)
    cons = exc._collision_block(eng, st, C, config, cs)
    assert np.array_equal(cons["g"], res["g"])
    # the capsule columns: what the capsule-only set returns through the existing path
    csel = np.nonzero(cols[:, 0] == 0)[0]
    if mode == "capsule":
        assert csel.size > 0
        only = exc.candidate_collision_gradient_from_coefficients(eng, cands, Tn, freq, config, {"capsules": cs["capsules"], "pairs": cs["pairs"],
                                                                                                   "margins": np.asarray(cs["margins"])[csel[np.argsort(cols[csel, 1])]]})
        order = csel[np.argsort(cols[csel, 1])]
        assert np.array_equal(only["g"], res["g"][:, order]) and np.array_equal(only["grad_q"], res["grad_q"][:, order])
        for k in only["grad"]:
            assert only["grad"][k].tobytes() == np.ascontiguousarray(res["grad"][k][:, order]).tobytes(), k
    else:
        assert csel.size == 0
    # the box rows against the restated chain
    bsel = np.nonzero(cols[:, 0] == 1)[0]
    q = st["q"].cpu().numpy()
    trans = (cons["idx"] < 0) & (cons["g"] < 1e10)
    assert trans[:, bsel].any(), "no transition configuration wins a box pair: choose another seed"
    c = int(np.argmax(trans[:, bsel].sum(axis=1)))
    flat = np.concatenate([res["grad"]["wf"][c][:, None], res["grad"]["q_offset"][c], res["grad"]["q_range"][c], res["grad"]["a"][c].reshape(P, -1),
                           res["grad"]["b"][c].reshape(P, -1)], axis=1)
    ref, want, bound = _restated_rows(topo, cs, cons, q, cands, c, freq, eps, bsel)
    err = np.abs(flat[bsel] - want)
    print(f"end to end {mode}: box rows against the restated chain: max |delta| / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}, max |row| = "
          f"{np.abs(want).max():.3f}; {int(trans[c, bsel].sum())} of {bsel.size} box pairs of candidate {c} won by a transition configuration")
    assert np.all(err <= bound)
    assert np.all(np.abs(res["grad_q"][c, bsel] - ref["grad"][c]) <= ref["bar"][c])
    assert np.abs(flat[bsel]).max() > 1e-3
    # central differences in the optimiser's variables, the evaluation points held fixed
    rows = exc.constraint_gradient_to_optimizer_variables({k: v[c] for k, v in res["grad"].items()}, cands[c], nf)
    assert rows.shape == (P, xs[c].size)
    order = bsel[np.argsort(cols[bsel, 1])]
    ev = {k: np.ascontiguousarray(np.asarray(cons[k])[c:c + 1, order]) for k in ("eval_sample", "eval_scale", "eval_pose")}
    eng.set_boxes(cs["boxes"], cs["box_pairs"], center_in_link_axes=bool(cs.get("center_in_link_axes", False)))
    margins = np.asarray(cs["margins"], dtype=np.float64)[order]

    def dist(x):
        s1 = exc.candidate_states(eng, [make(x)], Tn, freq, device=True)
        out = eng.box_distance_gradients(s1, 1, ev["eval_sample"], scale=ev["eval_scale"], pose_sample=ev["eval_pose"], epsilon=eps)
        return out["dist"].cpu().numpy()[0], s1["q"].cpu().numpy()

    from box_collision_restatement import index_boxes

    boxes = index_boxes(topo, cs["boxes"])
    bpairs = np.asarray(cs["box_pairs"]).reshape(-1, 2)
    lm = bool(cs.get("center_in_link_axes", False))

    def gap_sign(q1):
        r = bg.evaluate(topo, boxes, bpairs, False, q1, None, None, 1, ev["eval_sample"], ev["eval_scale"], ev["eval_pose"], eps, lm)
        return np.sign(r["gap"][0])

    base, q0 = dist(xs[c])
    won = ev["eval_sample"][0] >= 0
    assert np.abs(base - margins - res["g"][c, order])[won].max() <= 1e-12
    s0 = gap_sign(q0)
    keep = won.copy()
    fd = np.zeros((order.size, xs[c].size))
    for v in range(xs[c].size):
        xp, xm = xs[c].copy(), xs[c].copy()
        xp[v] += 1e-6
        xm[v] -= 1e-6
        (dp, qp), (dm, qm) = dist(xp), dist(xm)
        keep &= (gap_sign(qp) == s0) & (gap_sign(qm) == s0)
        fd[:, v] = (dp - dm) / 2e-6
    assert keep.sum() >= 0.9 * won.sum(), "more than 10 % of the box rows sit on a kink: choose another seed"
    err = np.abs(fd - rows[order])[keep]
    print(f"end to end {mode}: max |row - FD| = {err.max():.3e} over {int(keep.sum())} of {int(won.sum())} box rows, max |row| = {np.abs(rows[order][keep]).max():.3f}")
    assert err.max() <= FD_BAR
    eng.close()


def test_whole_gradient_with_box_rows():
    """candidate_gradients_from_coefficients(collision=cs, box_gradient=True): f, g, obj_grad and the non-collision rows of con_grad equal the
    call without collision, the collision rows equal candidate_collision_gradient's"""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from test_boxes import kuka_mixed_set
    from test_gpu_box_objectives import _cols

    rng = np.random.default_rng(12)
    topo, cs = kuka_mixed_set("capsule", rng, link_axes=True)
    eng = Engine(topo, floating=False)
    n, C, Tn, freq = topo.num_dofs, 2, 60, 20.0
    cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.4 for _ in range(n)], [rng.standard_normal(2) * 0.4 for _ in range(n)],
                                      rng.uniform(-0.2, 0.2, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 4, "collisionMode": "capsule"}
    icols = _cols(eng, topo, False)
    args = (eng, cands, Tn, freq, topo.x_std(), icols, limits, topo.dof_names, config)
    base = exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0)
    full = exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0, collision=cs, box_gradient=True)
    n0 = base["layout"]["len"]
    assert full["layout"]["collision"] == n0 and np.array_equal(full["f"], base["f"]) and np.array_equal(full["g"][:, :n0], base["g"])
    coll = exc.candidate_collision_gradient_from_coefficients(eng, cands, Tn, freq, config, cs, box_gradient=True)
    assert np.array_equal(full["g"][:, n0:], coll["g"])
    for k in base["obj_grad"]:
        assert np.array_equal(full["obj_grad"][k], base["obj_grad"][k]), k
        assert np.array_equal(full["con_grad"][k][:, :n0], base["con_grad"][k]), k
        assert np.array_equal(full["con_grad"][k][:, n0:], coll["grad"][k]), k
    assert np.abs(coll["grad"]["a"][:, np.asarray(cs["columns"])[:, 0] == 1]).max() > 1e-3
    with pytest.raises(ValueError, match="box pairs"):
        exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0, collision=cs)
    eng.close()
