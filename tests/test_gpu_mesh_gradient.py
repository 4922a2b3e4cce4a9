"""fbr_mesh_distance_gradients / Engine.mesh_distance_gradients and the mesh_gradient=True path of excitation on the device against the g++
emulation of the same text (the single pass: tests/emul/mesh_grad_emul.cpp) and the NumPy / Qhull restatement
(tests/mesh_gradient_restatement.py): per entry |delta grad| <= bar, bar = (b+ + b-) / (2 eps) with b+- = max(10 dev, 32 EPS scale) the bar of
the distances at the two stencil points (dev: the emulation's largest deviation from the restatement over the case's centre distances); the
centre distance within its bar; entries the stencil never touches exactly 0.0.  Every comparison first asserts that the restatement's signed
value is more than 100 bars from 0 at each stencil point of a mesh pair (tests/test_mesh_gradient.reference).

At C = 64 and 65 the restatement covers candidates 0, 63 and 64; the emulation covers all, and a candidate without a restated bar is held to
the emulation under the smallest bar an item of its pair can have, b+- = max(10 dev, 32 EPS (diam A + diam B)).

Largest |delta grad| / bar measured on an MI355X: 0.025 against the restatement over the 8 cases of the first test (threeLinks 0.015, the
left arm 0.025), 0.029 in the corner-rule test; every candidate of the batches of 64 and 65 within 0.13 of the smallest bar of the emulation;
the gantry rows agree with the emulation to the last digit printed."""
import numpy as np
import pytest

import mesh_gradient_restatement as mg
import test_mesh_gradient as tmg
from test_box_gradient import T, item_arrays

pytestmark = pytest.mark.gpu
ROBOTS = ("threeLinks", "walkman_left_arm")
_CASES, _ENGINES = {}, {}


def _case(robot):
    if robot not in _CASES:
        _CASES[robot] = tmg.make_case(robot, C=65, shift=tmg.SHIFT[robot])
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


def _pick(sub, cands):
    fl, Tn = sub["floating"], sub["q"].shape[0] // sub["C"]
    rows = np.concatenate([np.arange(c * Tn, (c + 1) * Tn) for c in cands])
    return dict(sub, C=len(cands), q=sub["q"][rows], rpy=sub["rpy"][rows] if fl else None, bp=sub["bp"][rows] if fl else None)


def _reference(sub, pairs, sample, scale, pose, eps, mode, meshes=None):
    """the restatement with its bars for the candidates it covers (all below 64, else 0, 63 and the last), the emulation for all"""
    C = sub["C"]
    cands = np.arange(C) if C < 64 else np.unique([0, 63, C - 1])
    ed, eg = tmg.emul_evaluate(sub, C, sample, scale, pose, eps, mode, pairs, meshes=meshes)
    part = _pick(sub, cands)
    cut = lambda a: None if a is None else np.asarray(a)[cands]  # noqa: E731
    meshes = sub["meshes"] if meshes is None else meshes
    ref = mg.evaluate(part["topo"], part["tuples"], meshes, pairs, part["floating"], part["q"], part["rpy"], part["bp"], len(cands), cut(sample),
                      cut(scale), cut(pose), eps, mode)
    fin = np.isfinite(ref["dist"]) & ~ref["none"]
    assert np.array_equal(np.isfinite(ref["dist"]), np.isfinite(ed[cands]))
    ref = mg.with_dev(ref, float(np.abs(ed[cands] - ref["dist"])[fin].max()) if fin.any() else 0.0)
    assert mg.clear_verdicts(ref).all(), "a stencil point of a mesh pair within 100 bars of contact: change the case"
    # the smallest bar an item of pair k can have: its scale is |c_B - c_A| + diam A + diam B
    diam = tmg.hg.diameters(sub["tuples"])
    low = np.maximum(10.0 * ref["dev"], 32.0 * mg.EPS * (diam[pairs[:, 0]] + diam[pairs[:, 1]]))
    return dict(ref, cands=cands, emul_dist=ed, emul_grad=eg, all_none=np.asarray(sample) < 0, low=low)


def _compare(got, ref, why):
    """the largest |delta grad| / bar, after the assertions"""
    cd, none, an = ref["cands"], ref["none"], ref["all_none"]
    assert got["dist"].shape == ref["emul_dist"].shape and got["grad_q"].shape == ref["emul_grad"].shape, why
    assert np.all(got["dist"][an] == mg.NONE) and np.all(got["grad_q"][an] == 0.0), why
    errd = (np.abs(got["dist"][cd] - ref["dist"]) / ref["dist_bar"])[~none]
    erre = (np.abs(got["dist"][cd] - ref["emul_dist"][cd]) / ref["dist_bar"])[~none]
    rel = np.abs(got["grad_q"][cd] - ref["grad"]) / ref["bar"]
    rele = np.abs(got["grad_q"][cd] - ref["emul_grad"][cd]) / ref["bar"]
    # every candidate against the emulation under the smallest bar an item can have
    low = ref["low"]
    alld = np.where(an, 0.0, np.abs(got["dist"] - ref["emul_dist"])) / low[None, :]
    allg = np.abs(got["grad_q"] - ref["emul_grad"]) / (low / ref["eps"])[None, :, None]
    print(f"{why}: max |delta dist| / bar = {errd.max() if errd.size else 0.0:.3f} (restatement) {erre.max() if erre.size else 0.0:.3f} (emulation), "
          f"max |delta grad| / bar = {rel.max():.4f} (restatement) {rele.max():.4f} (emulation); all candidates against the emulation: "
          f"{alld.max():.3f}, {allg.max():.4f} of the smallest bar")
    assert np.all(errd <= 1.0) and np.all(erre <= 1.0), why
    assert np.all(rel <= 1.0) and np.all(rele <= 1.0), why
    assert np.all(alld <= 1.0) and np.all(allg <= 1.0), why
    assert np.all(got["grad_q"][cd][~ref["on_path"]] == 0.0), why
    m = np.broadcast_to(ref["meshed"][None, :], got["dist"].shape) & ~an
    assert np.all(got["dist"][m] >= 0.0), why
    return float(rel.max())


def _states(sub, device):
    st = {"q": sub["q"]} if not sub["floating"] else {"q": sub["q"], "rpy": sub["rpy"]}
    return ({k: _cuda(v) for k, v in st.items()}, _cuda(sub["bp"])) if device else (st, sub["bp"])


def _select(case, classes):
    """the first pair of each of ``classes`` the case has"""
    return np.array([case["classes"].index(k) for k in classes if k in case["classes"]])


@pytest.mark.parametrize("eps", [1e-7, 1e-4])
@pytest.mark.parametrize("mode", [False, True], ids=["world-axes", "link-axes"])
@pytest.mark.parametrize("robot", ROBOTS)
def test_device_matches_the_emulation_and_the_restatement(robot, mode, eps):
    """C = 1 (one lane), 3 (a ragged wave), 64 (an exact wave), 65 (the tile boundary: a second wave of one lane); samples 0, T - 1, interior
    and -1 mixed; scale NULL and host arrays with host results (C = 1, 3), random scale and device tensors with device results (every C);
    pose_sample != sample.  The sets mix mesh-mesh, mesh-hull (either order), mesh-world (either order) and plain pairs.
    Every case prints its own figures; the largest are in the module's docstring."""
    case, eng = _case(robot), _engine(robot)
    rng = np.random.default_rng(21)
    allp = np.arange(len(case["pairs"]))
    worst = 0.0
    for C, sel in ((1, _select(case, ["mh"])), (3, allp), (64, _select(case, ["mm", "mh", "plain"])), (65, _select(case, ["hm", "mh", "wm", "plain"]))):
        pairs = case["pairs"][sel]
        P = len(pairs)
        sub = _sub(case, C)
        eng.set_hulls(case["hulls"], pairs, offset_in_link_axes=mode, meshes=case["meshes"])
        sample, scale, pose = item_arrays(sub, rng, C, P, True)
        why = f"{robot} mode {int(mode)} eps {eps:g} C{C} P{P}"
        if C < 64:
            st, bp = _states(sub, False)
            got = eng.mesh_distance_gradients(st, C, sample, pose_sample=pose, base_pos=bp, epsilon=eps)
            assert isinstance(got["dist"], np.ndarray) and got["grad_q"].shape == (C, P, case["topo"].num_dofs)
            worst = max(worst, _compare(got, _reference(sub, pairs, sample, None, pose, eps, mode), why + " scale NULL"))
        dst, dbp = _states(sub, True)
        gd = eng.mesh_distance_gradients(dst, C, _cuda(sample), scale=_cuda(scale), pose_sample=_cuda(pose), base_pos=dbp, epsilon=eps)
        assert hasattr(gd["dist"], "cpu")
        worst = max(worst, _compare(_host(gd), _reference(sub, pairs, sample, scale, pose, eps, mode), why + " random scale"))
        if C == 3:  # host states, device results; pose_sample None
            st, bp = _states(sub, False)
            mixed = eng.mesh_distance_gradients(st, C, sample, scale=scale, pose_sample=pose, base_pos=bp, epsilon=eps, device_out=True)
            assert hasattr(mixed["dist"], "cpu") and _host(mixed)["grad_q"].tobytes() == _host(gd)["grad_q"].tobytes()
            nop = _host(eng.mesh_distance_gradients(dst, C, _cuda(sample), scale=_cuda(scale), base_pos=dbp, epsilon=eps))
            _compare(nop, _reference(sub, pairs, sample, scale, None, eps, mode), why + " pose NULL")
    print(f"{robot} mode {int(mode)} eps {eps:g}: largest |delta grad| / bar = {worst:.4f}")


def test_corner_rules_and_determinism():
    """sample -1: 1e10 and a zero row; two calls give the same bytes; candidate c alone equals candidate c in the batch of 65; the pair list
    and the mesh list shuffled give the same bytes per pair; the plain pairs of the mixed set return the bytes of hull_distance_gradients on
    the set without meshes; candidate_hull_distances returns the same bytes before and after; a NaN row of q poisons that candidate's
    distances and evaluated entries only"""
    robot = "walkman_left_arm"
    case, eng = _case(robot), _engine(robot)
    C, P, eps, mode = 65, len(case["pairs"]), 1e-7, True
    sub = _sub(case, C)
    rng = np.random.default_rng(9)
    sample = rng.integers(0, T, (C, P)).astype(np.int64)
    sample[1, 2] = -1
    sample[3, :] = 4
    eng.set_hulls(case["hulls"], case["pairs"], offset_in_link_axes=mode, meshes=case["meshes"])
    st, bp = _states(sub, False)
    before = eng.candidate_hull_distances(st, C, 1, base_pos=bp)
    got = eng.mesh_distance_gradients(st, C, sample, base_pos=bp, epsilon=eps)
    again = eng.mesh_distance_gradients(st, C, sample, base_pos=bp, epsilon=eps)
    after = eng.candidate_hull_distances(st, C, 1, base_pos=bp)
    assert got["dist"].tobytes() == again["dist"].tobytes() and got["grad_q"].tobytes() == again["grad_q"].tobytes()
    assert before["dist"].tobytes() == after["dist"].tobytes() and before["idx"].tobytes() == after["idx"].tobytes()
    assert got["dist"][1, 2] == 1e10 and np.all(got["grad_q"][1, 2] == 0.0)
    _compare(got, _reference(sub, case["pairs"], sample, None, None, eps, mode), "corner rules")
    on = np.array([mg.path_dofs(case["topo"], case["tuples"][a][0], case["tuples"][b][0], mode) for a, b in case["pairs"]])
    assert np.all(got["grad_q"][:, ~on] == 0.0) and np.abs(got["grad_q"][:, on]).max() > 1e-2
    # one candidate alone
    for c in (0, 63, 64):
        one = _pick(sub, [c])
        s1, b1 = _states(one, False)
        alone = eng.mesh_distance_gradients(s1, 1, sample[c:c + 1], base_pos=b1, epsilon=eps)
        assert alone["dist"].tobytes() == got["dist"][c:c + 1].tobytes() and alone["grad_q"].tobytes() == got["grad_q"][c:c + 1].tobytes(), c
    # the pair list and the mesh list shuffled
    perm = rng.permutation(P)
    keys = list(case["meshes"])
    shuffled = {k: case["meshes"][k] for k in [keys[i] for i in rng.permutation(len(keys))]}
    eng.set_hulls(case["hulls"], case["pairs"][perm], offset_in_link_axes=mode, meshes=shuffled)
    sh = eng.mesh_distance_gradients(st, C, np.ascontiguousarray(sample[:, perm]), base_pos=bp, epsilon=eps)
    assert sh["dist"].tobytes() == np.ascontiguousarray(got["dist"][:, perm]).tobytes()
    assert sh["grad_q"].tobytes() == np.ascontiguousarray(got["grad_q"][:, perm]).tobytes()
    # the plain pairs: the bytes of the hull call on the set without meshes
    eng.set_hulls(case["hulls"], case["pairs"], offset_in_link_axes=mode)
    hull = eng.hull_distance_gradients(st, C, sample, base_pos=bp, epsilon=eps)
    plain = np.array([k == "plain" for k in case["classes"]])
    assert plain.any() and not plain.all()
    assert np.ascontiguousarray(hull["dist"][:, plain]).tobytes() == np.ascontiguousarray(got["dist"][:, plain]).tobytes()
    assert np.ascontiguousarray(hull["grad_q"][:, plain]).tobytes() == np.ascontiguousarray(got["grad_q"][:, plain]).tobytes()
    # a NaN in one candidate's q
    eng.set_hulls(case["hulls"], case["pairs"], offset_in_link_axes=mode, meshes=case["meshes"])
    qn = sub["q"].copy()
    qn[3 * T + 4] = np.nan  # the row every item of candidate 3 evaluates
    gn = eng.mesh_distance_gradients(dict(st, q=qn), C, sample, base_pos=bp, epsilon=eps)
    keep = np.arange(C) != 3
    assert gn["dist"][keep].tobytes() == got["dist"][keep].tobytes() and gn["grad_q"][keep].tobytes() == got["grad_q"][keep].tobytes()
    moved = on.any(axis=1)  # (a pair no joint moves -- a world hull against the base link's -- holds no NaN)
    assert np.all(np.isnan(gn["dist"][3][moved])) and np.all(np.isnan(gn["grad_q"][3][on])) and np.all(gn["grad_q"][3][~on] == 0.0) and (~on).any()


def test_invalid_arguments_are_refused():
    """an index of T and one of -2 each give FBR_E_INVALID and the next valid call on the same handle the bytes of the call before;
    set_hull_meshes({}) and then the mesh call: FBR_E_INVALID; the hull call on a set with meshes stays FBR_E_UNSUPPORTED"""
    from flobaroid_amd._lib import Engine, FbrError

    case = _case("threeLinks")
    topo, hulls, pairs = case["topo"], case["hulls"], case["pairs"]
    eng = Engine(topo, floating=False)
    P = len(pairs)
    sub = _sub(case, 2)
    st = {"q": sub["q"]}
    ok = np.zeros((2, P), dtype=np.int64)
    with pytest.raises(FbrError, match="code -1"):  # no hull set
        eng.mesh_distance_gradients(st, 2, np.zeros((2, 0), dtype=np.int64))
    eng.set_hulls(hulls, pairs, offset_in_link_axes=True)
    with pytest.raises(FbrError, match=r"code -1.*fbr_hull_distance_gradients"):  # no meshes attached
        eng.mesh_distance_gradients(st, 2, ok)
    eng.set_hulls(hulls, pairs, offset_in_link_axes=True, meshes=case["meshes"])
    first = eng.mesh_distance_gradients(st, 2, ok, epsilon=1e-7)
    with pytest.raises(FbrError, match=r"code -4.*triangle meshes attached"):  # FBR_E_UNSUPPORTED, as before
        eng.hull_distance_gradients(st, 2, ok)
    with pytest.raises(FbrError, match="code -1"):  # ncand < 1
        eng.mesh_distance_gradients(st, 0, np.zeros((1, P), dtype=np.int64))
    with pytest.raises(FbrError, match="code -1"):  # not a multiple
        eng.mesh_distance_gradients({"q": sub["q"][:13]}, 2, ok)
    for bad_sample, bad_pose, at in ((T, None, P - 1), (-2, None, 0), (T, None, 0), (-2, None, P - 1), (0, T, 0), (0, -5, P - 1)):
        s = ok.copy()
        s[1, at] = bad_sample  # (a mesh pair first, a plain pair last)
        pose = None
        if bad_pose is not None:
            pose = ok.copy()
            pose[0, at] = bad_pose
        with pytest.raises(FbrError, match="code -1"):
            eng.mesh_distance_gradients(st, 2, s, pose_sample=pose)
        nxt = eng.mesh_distance_gradients(st, 2, ok, epsilon=1e-7)
        assert nxt["dist"].tobytes() == first["dist"].tobytes() and nxt["grad_q"].tobytes() == first["grad_q"].tobytes()
    for bad in (0.0, -1e-7, float("nan"), float("inf")):
        with pytest.raises(FbrError, match="code -1"):
            eng.mesh_distance_gradients(st, 2, ok, epsilon=bad)
    _compare(first, _reference(sub, pairs, ok, None, None, 1e-7, True), "before the refused calls")
    eng.set_hull_meshes({})
    with pytest.raises(FbrError, match="code -1"):
        eng.mesh_distance_gradients(st, 2, ok)
    eng.close()


def test_gantry_contacts_on_the_device():
    """the apex 1e-2 above the mesh face: the row +-1 in the lift and 0 in the slide within the bar; 1e-3 through it: dist == 0.0 and a row
    that is exactly 0.0, the plain pairs of the same set keeping their depth and slope"""
    from flobaroid_amd._lib import Engine

    smp = np.zeros((1, 4), dtype=np.int64)
    eng = None
    for which in ("meshes", "meshes_hull"):
        for gap in (1e-2, -1e-3):
            case = tmg.gantry_case(gap)
            eng = eng or Engine(case["topo"], floating=False)
            for mode in (False, True):
                eng.set_hulls(case["hulls"], case["pairs"], offset_in_link_axes=mode, meshes=case[which])
                for eps in (1e-7, 1e-4):
                    got = eng.mesh_distance_gradients({"q": case["q"]}, 1, smp, epsilon=eps)
                    ref = _reference(case, case["pairs"], smp, None, None, eps, mode, meshes=case[which])
                    _compare(got, ref, f"gantry {which} gap {gap:g} mode {int(mode)} eps {eps:g}")
                    m = ref["meshed"]
                    if gap > 0:
                        assert np.all(np.abs(got["dist"][0] - gap) <= ref["dist_bar"][0]) and np.all(np.abs(got["grad_q"][0] - tmg.STACK_ROWS) <= ref["bar"][0])
                    else:
                        assert np.all(got["dist"][0][m] == 0.0) and np.all(got["grad_q"][0][m] == 0.0)
                        assert np.all(got["dist"][0][~m] < 0.0) and np.all(np.abs(got["grad_q"][0][~m] - tmg.STACK_ROWS[~m]) <= ref["bar"][0][~m])
    eng.close()


def test_mesh_gradient_end_to_end():
    """tests/test_mesh_gradient.e2e_case: kuka_lwr4 with two links served as meshes (fullMeshLinks) and the lifted floor, 3 candidates x 60
    samples, transitions on.  f and g of candidate_gradients_from_coefficients(collision=cs, mesh_gradient=True) are the bytes of
    candidate_objectives_from_coefficients, the non-collision rows those of the call without a collision set, the collision rows -- at
    layout["collision"] -- those of candidate_collision_gradient_from_coefficients; without the keyword the set is refused as before.  The
    collision rows of one candidate equal the restated chain within the chained bars; then every optimiser variable of that candidate is
    moved by +-1e-6, the DEVICE's collision block re-evaluated, and the central difference held against the
    constraint_gradient_to_optimizer_variables rows.

    E2E_FD_BAR = 5e-8: the same experiment with the restatement alone (tests/test_mesh_gradient.py
    test_end_to_end_seed_with_the_restatement_alone) gives 4.5e-9 on the committed seed, 13 of 14 rows kept (7 of the 8 mesh rows); x 10,
    rounded up.  Rows whose winning configuration changes on the stencil and rows whose centre distance is <= 0 are left out: a quarter at
    most (asserted).
    Measured on an MI355X: max |row - FD| = 4.7e-9 over 13 of 14 rows (7 mesh rows, max |row| 0.92); the rows within 0.027 of the chained
    bars of the restated chain."""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from test_gpu_box_objectives import _cols

    case = tmg.e2e_case()
    topo, cs, config, C, Tn, freq, nf = case["topo"], case["cs"], case["config"], case["C"], case["T"], case["freq"], case["nf"]
    eng = Engine(topo, floating=False)
    n, P = topo.num_dofs, len(cs["pair_names"])
    cands = [case["make"](x) for x in case["xs"]]
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    icols = _cols(eng, topo, False)
    args = (eng, cands, Tn, freq, topo.x_std(), icols, limits, topo.dof_names, config)
    full = exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0, collision=cs, mesh_gradient=True)
    obj = exc.candidate_objectives_from_coefficients(*args, dopt_scale=1.0, collision=cs)
    assert np.asarray(full["f"]).tobytes() == np.asarray(obj["f"]).tobytes() and np.asarray(full["g"]).tobytes() == np.asarray(obj["g"]).tobytes()
    base = exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0)
    n0 = full["layout"]["collision"]
    assert n0 == base["layout"]["len"] and full["g"].shape == (C, n0 + P)
    coll = exc.candidate_collision_gradient_from_coefficients(eng, cands, Tn, freq, config, cs, mesh_gradient=True)
    assert np.array_equal(coll["g"], full["g"][:, n0:]) and coll["grad_q"].shape == (C, P, n)
    for k in base["obj_grad"]:
        assert np.array_equal(full["obj_grad"][k], base["obj_grad"][k]), k
        assert np.array_equal(full["con_grad"][k][:, :n0], base["con_grad"][k]), k
        assert np.array_equal(full["con_grad"][k][:, n0:], coll["grad"][k]), k
    for kw in ({}, {"hull_gradient": True}):
        with pytest.raises(ValueError, match="triangle meshes"):
            exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0, collision=cs, **kw)
    # the collision rows against the restated chain
    st = exc.candidate_states(eng, cands, Tn, freq, device=True)
    cons = exc._collision_block(eng, st, C, config, cs)
    assert np.array_equal(cons["g"], coll["g"])
    q = st["q"].cpu().numpy()
    trans = (cons["idx"] < 0) & (cons["g"] < 1e10)
    assert trans.any(), "no transition configuration wins a pair: choose another seed"
    c = int(np.argmax(trans.sum(axis=1)))
    g = coll["grad"]
    flat = np.concatenate([g["wf"][c][:, None], g["q_offset"][c], g["q_range"][c], g["a"][c].reshape(P, -1), g["b"][c].reshape(P, -1)], axis=1)
    ref, want, bound = tmg.restated_rows(case, cons, q, cands, c, 1e-7)
    err = np.abs(flat - want)
    print(f"end to end: rows against the restated chain: max |delta| / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}, max |row| = "
          f"{np.abs(want).max():.3f}; {int(trans[c].sum())} of {P} pairs of candidate {c} won by a transition configuration")
    assert np.all(err <= bound) and np.all(np.abs(coll["grad_q"][c] - ref["grad"][c]) <= ref["bar"][c]) and np.abs(flat).max() > 1e-3
    # central differences of the device's block in the optimiser's variables
    rows = exc.constraint_gradient_to_optimizer_variables({k: v[c] for k, v in g.items()}, cands[c], nf)
    assert rows.shape == (P, case["xs"][c].size)
    margins = np.asarray(cs["margins"], dtype=np.float64)

    def block(x):
        s1 = exc.candidate_states(eng, [case["make"](x)], Tn, freq, device=True)
        b = exc._collision_block(eng, s1, 1, config, cs)
        return np.asarray(b["g"])[0], np.asarray(b["idx"])[0]

    fd, keep = tmg.thg.variable_differences(block, case["xs"][c], margins)
    errv = np.abs(fd - rows)[keep].max()
    print(f"end to end: max |row - FD| = {errv:.3e} over {int(keep.sum())} of {P} rows ({int((keep & ref['meshed']).sum())} mesh rows), "
          f"max |row| = {np.abs(rows[keep]).max():.3f}")
    assert keep.sum() >= (1.0 - tmg.E2E_MAX_EXCLUDED) * P, "more than a quarter of the rows are left out: choose another seed"
    assert (keep & ref["meshed"]).any() and errv <= tmg.E2E_FD_BAR
    eng.close()
