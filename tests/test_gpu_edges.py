"""Every kinematics route of the device against the long-double reference at state edges (tests/edge_reference.py): batches of equally
sized classes -- ordinary, at rest, exact angles, tiny, many turns, fast, hard acceleration, base attitude, friction edges -- laid out class
after class, so that waves, chunks and Gram images mix classes.  Every bar is scaled by the sample's (or the class's) own reference: a fast
sample cannot loosen the bar of a resting one.  The bar is the project's 1e-11 (edge_reference.class_bar: the double oracle stays below
1e-12 in every class, tests/test_edge_reference.py).  Worst ratios seen on an MI355X: DESIGN.md 2 ("Parity at state edges")."""
import functools

import numpy as np
import pytest

import edge_reference as er

pytestmark = pytest.mark.gpu

LD = np.longdouble
T = er.CLASS_SIZE
ROUTES = {
    "default": {},
    "fused_id0": {"fused_id": 0},
    "gram_lane0": {"gram_lane": 0},
    "link_merge0": {"link_merge": 0},
    "reduced": {"reduce_min_work": 0, "tsqr_group_min_samples": 1, "reduce_grouped_min_samples": 1},
    "chunk40": {"chunk_samples": 40},   # chunks cut classes
}
CASES = [(k, r) for k in er.CONFIG_KEYS for r in ROUTES]
case_ids = [f"{k}-{r}" for k, r in CASES]


def _engine(key, route):
    from flobaroid_amd._lib import Engine

    topo, floating, friction, stribeck = er.config(key)
    return Engine(topo, floating=floating, friction=friction, friction_symmetric=True, stribeck_velocity=stribeck, options=ROUTES[route])


def _report(key, route, what, by):
    print(f"edges | {key} | {route} | {what} | " + " ".join(f"{c}={r:.1e}" for c, r in by.items()))


def _assert_classes(key, route, what, by):
    for c, r in by.items():
        assert r <= er.class_bar(key, c), (key, route, what, c, r)


# ------------------------------------------------------------------------------------------------------------------------------------
# per-sample entry points
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fd_weights(key):
    ref = er.reference(key)
    W = np.random.default_rng([78, er.CONFIG_KEYS.index(key)]).standard_normal((ref["S"], ref["rows"], ref["P"]))
    base = (np.asarray(W, dtype=LD) * ref["Y"]).sum(axis=(1, 2))
    return W, base


def _per_sample(eng, key, st):
    """the five per-sample entry points on the states st, each (S, ...)"""
    ref = er.reference(key)
    est = er.engine_states(st)
    S = st["q"].shape[0]
    W, _ = _fd_weights(key)
    return {"regressor": eng.regressor(est).reshape(S, ref["rows"], ref["P"]),
            "inverse_dynamics": eng.inverse_dynamics(est, ref["x_std"], vel_sign=st.get("vel_sign")),
            "predict": eng.predict(est, ref["x_pred"]),
            "contact_torques": eng.contact_torques(est, ref["frame"], ref["wrench"]),
            "fd_scores_baseline": eng.fd_scores(est, W.reshape(S * ref["rows"], ref["P"]), 1e-6)[:, 0]}


def _per_sample_reference(key):
    ref = er.reference(key)
    return {"regressor": ref["Y"], "inverse_dynamics": ref["tau"], "predict": ref["pred"], "contact_torques": ref["contact"],
            "fd_scores_baseline": _fd_weights(key)[1]}


@pytest.mark.parametrize("key,route", CASES, ids=case_ids)
def test_per_sample_entry_points_match_long_double_sample_by_sample(key, route):
    """fbr_regressor_batch, fbr_inverse_dynamics_batch, fbr_predict, fbr_contact_torques and the baseline column of fbr_fd_scores:
    max|got[s] - ref[s]| <= bar max|ref[s]| for every sample."""
    ref = er.reference(key)
    eng = _engine(key, route)
    got = _per_sample(eng, key, ref["st"])
    eng.close()
    want = _per_sample_reference(key)
    results = {what: er.worst_by_class(er.per_sample_ratio(got[what], want[what]), ref["names"]) for what in got}
    for what, by in results.items():
        _report(key, route, what, by)
    for what, by in results.items():
        _assert_classes(key, route, what, by)


# ------------------------------------------------------------------------------------------------------------------------------------
# neighbours: a sample's result does not depend on what sits next to it
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,route", CASES, ids=case_ids)
def test_a_nan_or_fast_neighbour_leaves_every_other_sample_its_bits(key, route):
    """Sample 70 (exact-angle class, two samples before the tiny class begins) replaced by a state whose q, dq and rpy are NaN, then by a
    fast state: same size, same options, same route; every other sample keeps its bits, the replaced one is NaN / what the fast state
    gives."""
    ref = er.reference(key)
    st, s = ref["st"], er.REPLACED
    fast = er.class_slices(ref["names"])["fast"].start + 3
    eng = _engine(key, route)
    names = ("regressor", "inverse_dynamics", "predict", "contact_torques")
    base = _per_sample(eng, key, st)
    with_nan = _per_sample(eng, key, er.nan_state(st, s))
    with_fast = _per_sample(eng, key, er.with_sample(st, s, st, fast))
    eng.close()
    others = np.arange(ref["S"]) != s
    fb = ref["rows"] - st["q"].shape[1]
    want = _per_sample_reference(key)
    for what in names:
        assert np.isfinite(base[what]).all(), (what, "the batch itself")
        for other, tag in ((with_nan, "NaN"), (with_fast, "fast")):
            assert np.array_equal(other[what][others], base[what][others]), (key, route, what, f"a {tag} neighbour changed another sample")
        row = with_nan[what][s]
        if what in ("inverse_dynamics", "predict"):
            assert np.isnan(row).all(), (key, route, what)
        else:  # the regressor has structural zeros (and constant friction columns), the contact Jacobian rows of joints off the chain
            assert np.isnan(row.reshape(ref["rows"], -1)).any(axis=1).sum() >= (ref["rows"] if what == "regressor" else 1), (key, route, what)
            if what == "contact_torques":  # (the force rows of a floating base are the wrench's force itself, whatever the state)
                assert np.array_equal(row[:fb // 2], base[what][s][:fb // 2]) and np.all(np.isnan(row[fb // 2:]) | (row[fb // 2:] == 0)), (key, route, what)
        # the fast state in the exact-angle sample's place: what the reference gives for that state (the wrench stays sample 70's own)
        r = er.per_sample_ratio(with_fast[what][s][None], want[what][fast][None] if what != "contact_torques" else
                                er.contact_torques_ld(key, er.sample_states(st, [fast]), ref["frame"], ref["wrench"][[s]]))[0]
        assert r <= er.class_bar(key, "fast"), (key, route, what, r)
        if what != "contact_torques":
            assert np.abs(with_fast[what][s]).max() > 10 * np.abs(base[what][s]).max(), (key, route, what, "not fast-sized")


# ------------------------------------------------------------------------------------------------------------------------------------
# reductions: every class judged on its own norm
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gram_reference(key):
    """rhs (S * rows, 2): N(0, 1) x the class's own max|Y_ref|; a 0/1 row mask; per class the long-double A^T A of that class alone,
    A = [Y | rhs], without and with the mask."""
    ref = er.reference(key)
    rows, P, names = ref["rows"], ref["P"], ref["names"]
    rng = np.random.default_rng([79, er.CONFIG_KEYS.index(key)])
    rhs = rng.standard_normal((ref["S"], rows, 2))
    mask = (rng.random((ref["S"], rows)) < 0.7).astype(np.float64)
    G, Gm = {}, {}
    for c, sl in er.class_slices(names).items():
        rhs[sl] *= float(np.abs(ref["Y"][sl]).max())
        A = np.concatenate([ref["Y"][sl], np.asarray(rhs[sl], dtype=LD)], axis=2).reshape(T * rows, P + 2)
        G[c] = A.T @ A
        Am = A * np.asarray(mask[sl], dtype=LD).reshape(-1, 1)
        Gm[c] = Am.T @ Am
    return rhs.reshape(-1, 2), mask.reshape(-1), G, Gm


def _gram_ratio(G, Gref):
    Gref = np.asarray(Gref, dtype=LD)
    return float(np.sqrt(((np.asarray(G, dtype=LD) - Gref) ** 2).sum()) / np.sqrt((Gref ** 2).sum()))


@pytest.mark.parametrize("key,route", CASES, ids=case_ids)
def test_grouped_gram_per_class_against_long_double(key, route):
    """fbr_gram_grouped with the groups equal to the classes: two rhs columns and none, no weights and a 0/1 row mask; every group against
    the long-double A^T A of its class alone, norm(G_g - G_ref_g) <= 1e-11 norm(G_ref_g)."""
    ref = er.reference(key)
    names, P = ref["names"], ref["P"]
    rhs, mask, G, Gm = _gram_reference(key)
    est = er.engine_states(ref["st"])
    eng = _engine(key, route)
    runs = {"gram_grouped k=2": (eng.gram_grouped(est, len(names), rhs=rhs), G, P + 2),
            "gram_grouped k=0": (eng.gram_grouped(est, len(names)), G, P),
            "gram_grouped k=2 mask": (eng.gram_grouped(est, len(names), rhs=rhs, w=mask), Gm, P + 2)}
    eng.close()
    results = {what: {c: _gram_ratio(got[i], want[c][:n, :n]) for i, c in enumerate(names)} for what, (got, want, n) in runs.items()}
    for what, by in results.items():
        _report(key, route, what, by)
    for what, by in results.items():
        _assert_classes(key, route, what, by)


@pytest.mark.parametrize("key,route", CASES, ids=case_ids)
def test_gram_and_tsqr_of_each_class_alone(key, route):
    """fbr_gram_accumulate and fbr_tsqr over each class on its own -- its 24 samples, and the class repeated to 264 samples so that
    several waves run -- against the long-double Gram of the class (R^T R for the TSQR)."""
    ref = er.reference(key)
    names, rows = ref["names"], ref["rows"]
    rhs, _, G, _ = _gram_reference(key)
    eng = _engine(key, route)
    results = {f"{what} S={T * rep}": {} for what in ("gram", "tsqr") for rep in (1, 11)}
    for c, sl in er.class_slices(names).items():
        one = er.engine_states(er.sample_states(ref["st"], sl))
        rhs_c = rhs[sl.start * rows:sl.stop * rows]
        for rep in (1, 11):
            st = {k: np.ascontiguousarray(np.tile(v, (rep, 1))) for k, v in one.items()}
            r = np.ascontiguousarray(np.tile(rhs_c, (rep, 1)))
            results[f"gram S={T * rep}"][c] = _gram_ratio(eng.gram(st, rhs=r), rep * G[c])
            R = eng.tsqr(st, rhs=r)
            assert np.all(np.tril(R, -1) == 0)
            R = np.asarray(R, dtype=LD)
            results[f"tsqr S={T * rep}"][c] = _gram_ratio(R.T @ R, rep * G[c])
    eng.close()
    for what, by in results.items():
        _report(key, route, what, by)
    for what, by in results.items():
        _assert_classes(key, route, what, by)


# ------------------------------------------------------------------------------------------------------------------------------------
# extrema: the candidates are the classes
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,route", CASES, ids=case_ids)
def test_candidate_extrema_with_the_classes_as_candidates(key, route):
    """fbr_candidate_extrema: the indices are NumPy's argmin / argmax on the states and on the engine's own torques; the |tau| maxima are
    the long-double torques of the sample they point at, to that sample's bar."""
    ref = er.reference(key)
    st, names = ref["st"], ref["names"]
    est = er.engine_states(st)
    C, n = len(names), st["q"].shape[1]
    fb = ref["rows"] - n
    eng = _engine(key, route)
    tau = eng.inverse_dynamics(est, ref["x_std"], vel_sign=st.get("vel_sign"))
    got = eng.candidate_extrema(est, C, ref["x_std"], vel_sign=st.get("vel_sign"))
    eng.close()
    q3, dq3 = st["q"].reshape(C, T, n), np.abs(st["dq"].reshape(C, T, n))
    tq = np.abs(np.nan_to_num(tau.reshape(C, T, -1)[..., fb:]))
    want = {"q_min": q3.min(axis=1), "q_min_idx": q3.argmin(axis=1), "q_max": q3.max(axis=1), "q_max_idx": q3.argmax(axis=1),
            "dq_absmax": dq3.max(axis=1), "dq_absmax_idx": dq3.argmax(axis=1), "tau_absmax": tq.max(axis=1), "tau_absmax_idx": tq.argmax(axis=1)}
    for k, v in want.items():
        assert np.array_equal(got[k], v), (key, route, k)
    by = {}
    for c, name in enumerate(names):
        s = c * T + got["tau_absmax_idx"][c]                        # (n,) samples the maxima point at
        true = np.abs(ref["tau"][s, fb + np.arange(n)])
        scale = np.abs(ref["tau"][s]).max(axis=1)
        by[name] = float((np.abs(np.asarray(got["tau_absmax"][c], dtype=LD) - true) / scale).max())
    _report(key, route, "candidate_extrema tau_absmax", by)
    _assert_classes(key, route, "candidate_extrema tau_absmax", by)


# ------------------------------------------------------------------------------------------------------------------------------------
# capsule poses
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", er.CAPSULE_KEYS)
@pytest.mark.parametrize("route", ["default", "link_merge0", "chunk40"])
def test_capsule_poses_at_exact_angles_many_turns_and_every_attitude(key, route):
    """fbr_candidate_capsule_distances on the exact-angle, multi-turn and base-attitude classes.  Every sample as a candidate of its own:
    each pose's distances against tests/capsule_restatement.py at that sample's bar.  Then each class as one candidate: the minimum at the
    bar of the sample it points at, and the index equal to the restatement's wherever that is decided (its two best samples further apart
    than the bar); elsewhere the device's sample must be one of the undecided best."""
    topo, caps, pairs, st, dist, bar = er.capsule_case(key)
    eng = _engine(key, route)
    eng.set_capsules(caps, pairs)
    S = dist.shape[0]
    each = eng.candidate_capsule_distances(st, S, 1)
    cls = eng.candidate_capsule_distances(st, len(er.CAPSULE_CLASSES), 1)
    eng.close()
    assert np.array_equal(each["idx"], np.zeros_like(each["idx"]))
    ratio = (np.abs(each["dist"] - dist) / bar[:, None]).reshape(len(er.CAPSULE_CLASSES), -1).max(axis=1) * er.BAR
    _report(key, route, "capsule_distances per pose", dict(zip(er.CAPSULE_CLASSES, ratio)))
    d3 = dist.reshape(len(er.CAPSULE_CLASSES), T, -1)
    want_idx = d3.argmin(axis=1)
    und = er.undecided_pairs(dist, bar)
    print(f"edges | {key} | {route} | capsule pairs left undecided | " + " ".join(f"{c}={u:.3f}" for c, u in zip(er.CAPSULE_CLASSES, und.mean(axis=1))))
    assert np.all(ratio <= er.BAR), (key, route, ratio)
    assert np.array_equal(cls["idx"][~und], want_idx[~und]), (key, route, "a decided winner differs")
    b3 = bar.reshape(len(er.CAPSULE_CLASSES), T)
    c, k = np.nonzero(np.ones_like(und))
    at = d3[c, cls["idx"][c, k], k]        # the restatement's distance at the device's sample
    assert np.all(np.abs(cls["dist"][c, k] - at) <= b3[c, cls["idx"][c, k]]), (key, route, "class minimum")
    assert np.all(at - d3.min(axis=1)[c, k] <= b3.max(axis=1)[c]), (key, route, "the device's sample is not among the best")
