"""fbr_hull_distance_gradients / Engine.hull_distance_gradients and the hull_gradient=True path of excitation on the device against the g++
emulation of the same text and the NumPy / Qhull restatement (tests/hull_gradient_restatement.py: whole re-walks at q +- eps e_d for every
joint, the Minkowski difference handed to Qhull): per entry |delta grad| <= bar, bar = (b+ + b-) / (2 eps) with b+- = max(10 dev, 32 EPS
scale) the bar of the hull distances at the two stencil points (dev: the emulation's largest deviation from the restatement over the
case's centre distances); the distance within its bar of the restatement and of the emulation; entries the stencil never touches exactly 0.0.

Largest |delta grad| / bar measured on an MI355X over the 16 cases (four robots, both offset modes, both steps): 0.048 (kuka_lwr4, offsets in
world axes, eps = 1e-7); per robot threeLinks 0.023, kuka_lwr4 0.048, walkman_left_arm 0.033, random tree 0.020 (every case prints its
own); against the emulation of the same text the gantry contacts agree to the last digit printed."""
import numpy as np
import pytest

import hull_gradient_restatement as hg
from test_box_gradient import ROBOTS, T, item_arrays
from test_hull_gradient import (E2E_FD_BAR, E2E_MAX_EXCLUDED, STACK_ROWS, e2e_case, emul_evaluate, gantry_case, make_case, restated_rows, small_hull,
                                variable_differences)

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
    """the restatement with its bars, and the emulation's distances on the same items"""
    C = sub["C"]
    ref = hg.evaluate(sub["topo"], sub["tuples"], pairs, sub["floating"], sub["q"], sub["rpy"], sub["bp"], C, sample, scale, pose, eps, mode)
    ed, eg = emul_evaluate(sub, C, sample, scale, pose, eps, mode, pairs)
    fin = np.isfinite(ref["dist"]) & ~ref["none"]
    assert np.array_equal(np.isfinite(ref["dist"]), np.isfinite(ed))
    ref = hg.with_dev(ref, float(np.abs(ed - ref["dist"])[fin].max()) if fin.any() else 0.0)
    return dict(ref, emul_dist=ed, emul_grad=eg)


def _compare(got, ref, why):
    """the largest |delta grad| / bar, after the assertions"""
    none = ref["none"]
    assert got["dist"].shape == ref["dist"].shape and got["grad_q"].shape == ref["grad"].shape, why
    assert np.all(got["dist"][none] == hg.NONE) and np.all(got["grad_q"][none] == 0.0), why
    errd = (np.abs(got["dist"] - ref["dist"]) / ref["dist_bar"])[~none]
    erre = (np.abs(got["dist"] - ref["emul_dist"]) / ref["dist_bar"])[~none]
    rel = np.abs(got["grad_q"] - ref["grad"]) / ref["bar"]
    rele = np.abs(got["grad_q"] - ref["emul_grad"]) / ref["bar"]
    print(f"{why}: max |delta dist| / bar = {errd.max() if errd.size else 0.0:.3f} (restatement) {erre.max() if erre.size else 0.0:.3f} (emulation), "
          f"max |delta grad| / bar = {rel.max():.4f} (restatement) {rele.max():.4f} (emulation)")
    assert np.all(errd <= 1.0) and np.all(erre <= 1.0), why
    assert np.all(rel <= 1.0) and np.all(rele <= 1.0), why
    assert np.all(got["grad_q"][~ref["on_path"]] == 0.0), why
    return float(rel.max())


def _states(sub, device):
    st = {"q": sub["q"]} if not sub["floating"] else {"q": sub["q"], "rpy": sub["rpy"]}
    return ({k: _cuda(v) for k, v in st.items()}, _cuda(sub["bp"])) if device else (st, sub["bp"])


@pytest.mark.parametrize("eps", [1e-7, 1e-4])
@pytest.mark.parametrize("mode", [False, True], ids=["world-axes", "link-axes"])
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_device_matches_the_emulation_and_the_restatement(robot, mode, eps):
    """C = 1 (one lane), 3 (a ragged wave), 64 (an exact wave), 65 (a wave never spans two pairs; 2 and 3 pairs there); samples 0, T - 1,
    interior and -1 mixed; scale NULL with host arrays (C = 1, 3) and random in (0, 1] with device tensors (every C); pose_sample != sample"""
    case, eng = _case(robot), _engine(robot)
    rng = np.random.default_rng(21)
    allp = case["pairs"]
    worst = 0.0
    for C, P in ((1, 1), (1, len(allp)), (3, len(allp)), (64, 2), (65, 3)):
        pairs = allp[np.sort(rng.choice(len(allp), P, replace=False))] if P < len(allp) else allp
        sub = _sub(case, C)
        eng.set_hulls(case["hulls"], pairs, offset_in_link_axes=mode)
        sample, scale, pose = item_arrays(sub, rng, C, P, True)
        why = f"{robot} mode {int(mode)} eps {eps:g} C{C} P{P}"
        if C < 64:
            st, bp = _states(sub, False)
            got = eng.hull_distance_gradients(st, C, sample, pose_sample=pose, base_pos=bp, epsilon=eps)
            assert isinstance(got["dist"], np.ndarray) and got["grad_q"].shape == (C, P, case["topo"].num_dofs)
            worst = max(worst, _compare(got, _reference(sub, pairs, sample, None, pose, eps, mode), why + " scale NULL"))
        dst, dbp = _states(sub, True)
        gd = eng.hull_distance_gradients(dst, C, _cuda(sample), scale=_cuda(scale), pose_sample=_cuda(pose), base_pos=dbp, epsilon=eps)
        assert hasattr(gd["dist"], "cpu")
        worst = max(worst, _compare(_host(gd), _reference(sub, pairs, sample, scale, pose, eps, mode), why + " random scale"))
    print(f"{robot} mode {int(mode)} eps {eps:g}: largest |delta grad| / bar = {worst:.4f}")


def test_corner_rules():
    """two hulls on one link (offsets in link axes): zero rows and a finite distance; sample -1: 1e10 and a zero row; two runs give the same
    bytes; a NaN row of q poisons that candidate's items only, and its untouched entries are still exactly 0; the distances of
    fbr_candidate_hull_distances are the same bytes before and after"""
    case, eng = _case("kuka_lwr4"), _engine("kuka_lwr4")
    hulls = list(case["hulls"])
    hulls.append(small_hull(np.random.default_rng(2), 0, hulls[4].link_name, np.array([0.05, 0.04, 0.03]), np.array([0.3, 0.0, 0.1])))
    pairs = np.concatenate([case["pairs"][:6], [[4, len(hulls) - 1]]]).astype(np.int32)
    C, P, eps = 4, len(pairs), 1e-7
    from test_hulls import as_tuples

    sub = dict(_sub(case, C), hulls=hulls, tuples=as_tuples(case["topo"], hulls))
    rng = np.random.default_rng(9)
    sample = rng.integers(0, T, (C, P)).astype(np.int64)
    sample[1, 2] = -1
    sample[3, :] = 4
    eng.set_hulls(hulls, pairs, offset_in_link_axes=True)
    st = {"q": sub["q"]}
    before = eng.candidate_hull_distances(st, C, 1)
    got = eng.hull_distance_gradients(st, C, sample, epsilon=eps)
    ref = _reference(sub, pairs, sample, None, None, eps, True)
    _compare(got, ref, "corner rules")
    assert np.all(got["grad_q"][:, P - 1] == 0.0) and np.all(np.isfinite(got["dist"][:, P - 1])) and not ref["on_path"][:, P - 1].any()
    assert got["dist"][1, 2] == 1e10 and np.all(got["grad_q"][1, 2] == 0.0)
    again = eng.hull_distance_gradients(st, C, sample, epsilon=eps)
    assert got["dist"].tobytes() == again["dist"].tobytes() and got["grad_q"].tobytes() == again["grad_q"].tobytes()
    after = eng.candidate_hull_distances(st, C, 1)
    assert before["dist"].tobytes() == after["dist"].tobytes() and before["idx"].tobytes() == after["idx"].tobytes()
    qn = sub["q"].copy()
    qn[3 * T + 4] = np.nan  # the row every item of candidate 3 evaluates
    gn = eng.hull_distance_gradients({"q": qn}, C, sample, epsilon=eps)
    assert np.array_equal(gn["dist"][:3], got["dist"][:3]) and np.array_equal(gn["grad_q"][:3], got["grad_q"][:3])
    # pair 4 is a world hull against the hull of the base link, which no joint moves: its poses hold no NaN
    assert sub["tuples"][pairs[4, 0]][0] < 0 and sub["tuples"][pairs[4, 1]][0] == 0
    moved = np.arange(P) != 4
    assert np.all(np.isnan(gn["dist"][3][moved])) and gn["dist"][3, 4] == got["dist"][3, 4]
    assert np.all(np.isnan(gn["grad_q"][3][ref["on_path"][3]]))
    assert np.all(gn["grad_q"][3][~ref["on_path"][3]] == 0.0) and (~ref["on_path"][3]).any()


def test_invalid_arguments_are_refused():
    from flobaroid_amd._lib import Engine, FbrError

    case = _case("kuka_lwr4")
    topo, hulls, pairs = case["topo"], case["hulls"], case["pairs"]
    eng = Engine(topo, floating=False)
    P = len(pairs)
    sub = _sub(case, 2)
    st = {"q": sub["q"]}
    ok = np.zeros((2, P), dtype=np.int64)
    with pytest.raises(FbrError, match="code -1"):  # no hull set
        eng.hull_distance_gradients(st, 2, np.zeros((2, 0), dtype=np.int64))
    eng.set_hulls(hulls, np.zeros((0, 2)))
    with pytest.raises(FbrError, match="code -1"):  # a set without pairs
        eng.hull_distance_gradients(st, 2, np.zeros((2, 0), dtype=np.int64))
    eng.set_hulls(hulls, pairs, offset_in_link_axes=True)
    with pytest.raises(FbrError, match="code -1"):  # ncand < 1
        eng.hull_distance_gradients(st, 0, np.zeros((1, P), dtype=np.int64))
    with pytest.raises(FbrError, match="code -1"):  # not a multiple
        eng.hull_distance_gradients({"q": sub["q"][:13]}, 2, ok)
    for bad_sample, bad_pose in ((T, None), (-2, None), (10**12, None), (0, T), (0, -5)):
        s = ok.copy()
        s[1, P - 1] = bad_sample
        pose = None
        if bad_pose is not None:
            pose = ok.copy()
            pose[0, 0] = bad_pose
        with pytest.raises(FbrError, match="code -1"):
            eng.hull_distance_gradients(st, 2, s, pose_sample=pose)
    for bad in (0.0, -1e-7, float("nan"), float("inf")):
        with pytest.raises(FbrError, match="code -1"):
            eng.hull_distance_gradients(st, 2, ok, epsilon=bad)
    got = eng.hull_distance_gradients(st, 2, ok, epsilon=1e-7)
    _compare(got, _reference(sub, pairs, ok, None, None, 1e-7, True), "after refused calls")
    eng.close()


def test_gantry_contacts_on_the_device():
    """parallel faces stacked along the lift axis 1e-2 apart and 1e-3 deep: the distance is the gap, the row +-1 in the lift and 0 in the
    slide within the bar; the 128-point sphere inside the 64-gon prisms: the largest tables"""
    from flobaroid_amd._lib import Engine

    smp = np.zeros((1, 4), dtype=np.int64)
    eng = None
    for kind, gap in (("stack", 1e-2), ("stack", -1e-3), ("round", 0.0)):
        case = gantry_case(kind, gap)
        eng = eng or Engine(case["topo"], floating=False)
        for mode in (False, True):
            eng.set_hulls(case["hulls"], case["pairs"], offset_in_link_axes=mode)
            for eps in (1e-7, 1e-4):
                got = eng.hull_distance_gradients({"q": case["q"]}, 1, smp, epsilon=eps)
                ref = _reference(case, case["pairs"], smp, None, None, eps, mode)
                _compare(got, ref, f"gantry {kind} gap {gap:g} mode {int(mode)} eps {eps:g}")
                if kind == "stack":
                    assert np.all(np.abs(got["dist"][0] - gap) <= ref["dist_bar"][0]) and np.all(np.abs(got["grad_q"][0] - STACK_ROWS) <= ref["bar"][0])
                else:
                    assert np.all(got["dist"] < -1e-2) and np.abs(got["grad_q"]).max() > 0.1
    eng.close()


def test_hull_gradient_end_to_end():
    """test_hull_gradient.e2e_case: kuka_lwr4 with box hulls and the lifted floor, 3 candidates x 60 samples, transitions on.  f and g of
    candidate_gradients_from_coefficients(collision=cs, hull_gradient=True) are the bytes of candidate_objectives_from_coefficients, the
    non-collision rows those of the call without a collision set, the collision rows those of candidate_collision_gradient_from_coefficients;
    the collision rows of one candidate equal the restated chain within the chained bars; then every optimiser variable of that candidate
    is moved by +-1e-6, the DEVICE's collision block re-evaluated, and the central difference held against the
    constraint_gradient_to_optimizer_variables rows.

    E2E_FD_BAR = 5e-8: the same experiment with the Qhull restatement alone (tests/test_hull_gradient.py
    test_end_to_end_seed_with_the_restatement_alone) gives 4.2e-9 on the committed seed, 13 of 14 rows kept; x 10, rounded up.  Rows whose
    winning configuration changes on the stencil, and rows whose centre distance is <= 0, are left out: a quarter at most (asserted).
    Measured on an MI355X: max |row - FD| = 3.9e-9 over 13 of 14 rows (max |row| 1.7); the rows within 0.027 of the chained bars of the
    restated chain."""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from test_gpu_box_objectives import _cols

    case = e2e_case()
    topo, cs, config, C, Tn, freq, nf = case["topo"], case["cs"], case["config"], case["C"], case["T"], case["freq"], case["nf"]
    eng = Engine(topo, floating=False)
    n, P = topo.num_dofs, len(cs["pair_names"])
    cands = [case["make"](x) for x in case["xs"]]
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    icols = _cols(eng, topo, False)
    args = (eng, cands, Tn, freq, topo.x_std(), icols, limits, topo.dof_names, config)
    full = exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0, collision=cs, hull_gradient=True)
    obj = exc.candidate_objectives_from_coefficients(*args, dopt_scale=1.0, collision=cs)
    assert np.asarray(full["f"]).tobytes() == np.asarray(obj["f"]).tobytes() and np.asarray(full["g"]).tobytes() == np.asarray(obj["g"]).tobytes()
    base = exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0)
    n0 = full["layout"]["collision"]
    assert n0 == base["layout"]["len"] and full["g"].shape == (C, n0 + P)
    coll = exc.candidate_collision_gradient_from_coefficients(eng, cands, Tn, freq, config, cs, hull_gradient=True)
    assert np.array_equal(coll["g"], full["g"][:, n0:]) and coll["grad_q"].shape == (C, P, n)
    for k in base["obj_grad"]:
        assert np.array_equal(full["obj_grad"][k], base["obj_grad"][k]), k
        assert np.array_equal(full["con_grad"][k][:, :n0], base["con_grad"][k]), k
        assert np.array_equal(full["con_grad"][k][:, n0:], coll["grad"][k]), k
    with pytest.raises(ValueError, match="hull pairs"):
        exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0, collision=cs)
    # the hull distances before and after a gradient call: the same bytes
    st = exc.candidate_states(eng, cands, Tn, freq, device=True)
    cons = exc._collision_block(eng, st, C, config, cs)
    assert np.array_equal(cons["g"], coll["g"])
    before = _host(eng.candidate_hull_distances(st, C, 3))
    order = np.argsort(np.asarray(cs["columns"])[:, 1], kind="stable")
    ev = [np.ascontiguousarray(np.asarray(cons[k])[:, order]) for k in ("eval_sample", "eval_scale", "eval_pose")]
    dg = _host(eng.hull_distance_gradients(st, C, ev[0], scale=ev[1], pose_sample=ev[2], epsilon=1e-7))
    after = _host(eng.candidate_hull_distances(st, C, 3))
    assert before["dist"].tobytes() == after["dist"].tobytes() and before["idx"].tobytes() == after["idx"].tobytes()
    won = ev[0] >= 0
    margins = np.asarray(cs["margins"], dtype=np.float64)
    assert np.abs(dg["dist"] - margins[order][None] - cons["g"][:, order])[won].max() <= 1e-12
    assert np.array_equal(dg["grad_q"], coll["grad_q"][:, order])
    # the collision rows against the restated chain
    q = st["q"].cpu().numpy()
    trans = (cons["idx"] < 0) & (cons["g"] < 1e10)
    assert trans.any(), "no transition configuration wins a pair: choose another seed"
    c = int(np.argmax(trans.sum(axis=1)))
    g = coll["grad"]
    flat = np.concatenate([g["wf"][c][:, None], g["q_offset"][c], g["q_range"][c], g["a"][c].reshape(P, -1), g["b"][c].reshape(P, -1)], axis=1)
    ref, want, bound = restated_rows(case, cons, q, cands, c, 1e-7)
    err = np.abs(flat - want)
    print(f"end to end: rows against the restated chain: max |delta| / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}, max |row| = "
          f"{np.abs(want).max():.3f}; {int(trans[c].sum())} of {P} pairs of candidate {c} won by a transition configuration")
    assert np.all(err <= bound) and np.all(np.abs(coll["grad_q"][c] - ref["grad"][c]) <= ref["bar"][c]) and np.abs(flat).max() > 1e-3
    # central differences of the device's block in the optimiser's variables
    rows = exc.constraint_gradient_to_optimizer_variables({k: v[c] for k, v in g.items()}, cands[c], nf)
    assert rows.shape == (P, case["xs"][c].size)

    def block(x):
        s1 = exc.candidate_states(eng, [case["make"](x)], Tn, freq, device=True)
        b = exc._collision_block(eng, s1, 1, config, cs)
        return np.asarray(b["g"])[0], np.asarray(b["idx"])[0]

    fd, keep = variable_differences(block, case["xs"][c], margins)
    errv = np.abs(fd - rows)[keep].max()
    print(f"end to end: max |row - FD| = {errv:.3e} over {int(keep.sum())} of {P} rows, max |row| = {np.abs(rows[keep]).max():.3f}")
    assert keep.sum() >= (1.0 - E2E_MAX_EXCLUDED) * P, "more than a quarter of the rows are left out: choose another seed"
    assert errv <= E2E_FD_BAR
    eng.close()
