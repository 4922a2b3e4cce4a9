"""The edge batches and their long-double reference (tests/edge_reference.py), pinned without a GPU: the double oracle against the
reference per sample, max|Y_o[s] - Y_ref[s]| / max|Y_ref[s]|, class by class.  The worst ratios are the figures of DESIGN.md 2 ("Parity at state edges") and the
baseline of the per-class bars of tests/test_gpu_edges.py."""
import numpy as np
import pytest

import edge_reference as er
import np_dynamics as nd
from oracle.oracle import OracleModel

LD = np.longdouble


def _oracle(key):
    topo, floating, friction, stribeck = er.config(key)
    return OracleModel(topo, floating=floating, fric=friction, fric_sym=True, stribeck=stribeck)


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than double on this platform: the reference would prove nothing"


@pytest.mark.parametrize("key", er.CONFIG_KEYS)
def test_the_batch_holds_every_class(key):
    topo, floating, friction, stribeck = er.config(key)
    st, names = er.edge_batch(key)
    want = ["ordinary", "rest", "exact", "tiny", "multiturn", "fast", "hardacc"] + ["attitude"] * floating + ["friction"] * friction
    assert names == want
    S = len(names) * er.CLASS_SIZE
    assert all(v.shape[0] == S for v in st.values()) and er.REPLACED < S
    # the first two 64-sample wave boundaries cut a class (8 classes give S = 192, three whole waves; 9 give 216 and a partial wave)
    assert 64 % er.CLASS_SIZE and 128 % er.CLASS_SIZE and len(names) in (8, 9)
    sl = er.class_slices(names)
    assert not st["dq"][sl["rest"]].any() and not st["ddq"][sl["rest"]].any()
    assert np.signbit(st["q"][sl["exact"]][0]).all() and not st["q"][sl["exact"]][0].any()
    assert set(np.abs(st["q"][sl["exact"]]).ravel()) <= {0.0, np.pi / 2, np.pi}
    assert 5e-324 in st["q"][sl["tiny"]] and -1e-310 in st["dq"][sl["tiny"]] and np.abs(st["q"][sl["tiny"]]).max() <= 1e-8
    assert np.abs(st["q"][sl["multiturn"]]).max() > 6e5 or topo.num_dofs == 0
    assert np.abs(st["dq"][sl["fast"]]).max() > 500 and np.abs(st["ddq"][sl["hardacc"]]).max() > 5e4
    if floating:
        assert not st["base_vel"][sl["rest"]].any() and not st["base_acc"][sl["rest"]].any()
        rpy = st["rpy"][sl["attitude"]]
        assert (rpy[:, 1] == np.pi / 2).sum() == 3 and (rpy[:, 1] == -np.pi / 2).sum() == 3 and (rpy < 0).any(axis=0).all()
        assert (st["base_vel"][sl["attitude"]] < 0).any(axis=0).all() and (st["base_vel"][sl["attitude"]] > 0).any(axis=0).all()
        # what the rest of the suite draws, for contrast: small positive attitudes, positive twists
        assert st["rpy"][sl["ordinary"]].min() >= 0 and st["rpy"][sl["ordinary"]].max() <= 0.1 and st["base_vel"][sl["ordinary"]].min() >= 0
    if friction:
        f = sl["friction"]
        assert set(st["sign"][f].ravel()) == {0.0, 1.0, -1.0} and (st["dq"][f] == 0).any() and (np.abs(st["dq"][f]) == 1e-12).any()
        if stribeck > 0:
            assert (np.exp(-np.abs(st["dq"][f]) / stribeck) == 0).any(), "no Stribeck term underflows"


@pytest.mark.parametrize("key", er.CONFIG_KEYS)
def test_reference_formulations_agree_and_vanish_at_zero_parameters(key):
    """The origin-based wrenches (linear in the parameters) against np_dynamics' centre-of-mass Newton-Euler, both in long double, at the
    topology's own parameters; gravity is mass-proportional, so nothing is left at x = 0; and Y_ref x = the torques of x.  The two
    formulations are the same function only for exactly orthonormal rest rotations and unit axes (R (c.c) 1 R^T = |R c|^2 1); those are
    doubles, orthonormal to 1e-16, and that defect -- not long double's rounding of 5e-20 -- is what is left between them: at most
    1.5e-16 of a sample's largest torque in the fast class (seen), bar 2e-15.  A robot is not defined more finely than that."""
    topo, floating, friction, stribeck = er.config(key)
    ref = er.reference(key)
    st = ref["st"]
    x = np.concatenate([topo.x_std(), np.zeros(ref["P"] - 10 * topo.num_links)])
    tau = er.torques_ld(key, st, x)
    assert tau.dtype == LD
    com = nd.inverse_dynamics_world(topo, st["q"], st["dq"], st["ddq"], floating, st.get("base_vel"), st.get("base_acc"), st.get("rpy"), dtype=LD)
    assert com.dtype == LD
    assert er.per_sample_ratio(tau, com).max() <= 2e-15
    assert not er.torques_ld(key, st, np.zeros(ref["P"])).any()
    if not (friction and stribeck > 0):  # (the Stribeck torque takes vel_sign and sgn(sign), its regressor column dq: two different things)
        assert er.per_sample_ratio(np.einsum("srp,p->sr", ref["Y"], np.asarray(ref["x_std"], dtype=LD)), ref["tau"]).max() <= 1e-17
    # float64 stays float64, bit for bit what the default gives
    a = nd.inverse_dynamics_world(topo, st["q"], st["dq"], st["ddq"], floating, st.get("base_vel"), st.get("base_acc"), st.get("rpy"))
    b = nd.inverse_dynamics_world(topo, st["q"], st["dq"], st["ddq"], floating, st.get("base_vel"), st.get("base_acc"), st.get("rpy"),
                                  dtype=np.float64)
    assert a.dtype == np.float64 and np.array_equal(a, b)


def test_gravity_only_and_asymmetric_columns_by_indexing():
    """The two layouts no edge configuration uses, against the oracle on the ordinary class: 4 columns per link + the Coulomb block, and
    the split viscous columns."""
    key = "kuka-fric-st0.05"
    topo, floating, friction, stribeck = er.config(key)
    st = er.sample_states(er.reference(key)["st"], slice(0, er.CLASS_SIZE))
    est = er.engine_states(st)
    for kw, okw in (({"gravity_only": True}, {"grav_only": True}), ({"friction_symmetric": False}, {"fric_sym": False})):
        Y = er.regressor_ld(key, st, **kw)
        om = OracleModel(topo, floating=floating, fric=True, stribeck=stribeck, **okw)
        Yo = om.regressor(est, est["sign"]).reshape(Y.shape)
        assert er.per_sample_ratio(Yo, Y).max() <= er.ORACLE_CLEAN, kw


@pytest.mark.parametrize("key", er.CONFIG_KEYS)
def test_oracle_against_the_long_double_reference_per_sample(key):
    ref = er.reference(key)
    st, names = ref["st"], ref["names"]
    est = er.engine_states(st)
    om = _oracle(key)
    got = {"regressor": om.regressor(est, est.get("sign")).reshape(ref["Y"].shape),
           "inverse_dynamics": om.inverse_dynamics(est, ref["x_std"], est.get("sign"), st.get("vel_sign")),
           "contact_torques": om.contact_torques(est, ref["frame"], ref["wrench"])}
    want = {"regressor": ref["Y"], "inverse_dynamics": ref["tau"], "contact_torques": ref["contact"]}
    worst = {c: 0.0 for c in names}
    for what in got:
        by = er.worst_by_class(er.per_sample_ratio(got[what], want[what]), names)
        print(f"oracle / long double, {key}, {what}: " + "  ".join(f"{c} {r:.1e}" for c, r in by.items()))
        for c, r in by.items():
            worst[c] = max(worst[c], r)
    for c, r in worst.items():
        pinned = er.ORACLE_RATIO.get((key, c), 0.0)
        assert r <= max(pinned, er.ORACLE_CLEAN), (key, c, r, "the oracle's ratio is above what edge_reference.ORACLE_RATIO records")
        assert pinned == 0.0 or r >= pinned / 4, (key, c, r, "ORACLE_RATIO records far more than the oracle shows: the device bar is loose")


@pytest.mark.parametrize("key", er.CAPSULE_KEYS)
def test_capsule_winners_are_decided_on_the_restatement_alone(key):
    """The share of pairs whose winner the restatement leaves to rounding (its two best samples within the bar of each other): at most 2 %
    per class -- repeated poses aside.  Two classes repeat poses by construction: exact angles (six values, four distinct joint poses, 24
    samples) and the prismatic joints of the multi-turn class (+-50), and a pair of capsules sees only the joints on the chain between its
    links.  Such a pair is an exact tie of two equal poses, which the device test still checks (its sample must be one of the best); any
    other undecided pair counts against the 2 %."""
    topo, caps, pairs, st, dist, bar = er.capsule_case(key)
    und = er.undecided_pairs(dist, bar)
    anc = topo.ancestors_dofs()
    T = er.CLASS_SIZE
    for i, c in enumerate(er.CAPSULE_CLASSES):
        q = st["q"][i * T:(i + 1) * T]
        canon = np.where(np.abs(q) == np.pi, np.pi, q + 0.0)  # (-0.0 -> 0.0, -pi -> pi: the same pose to 2.4e-16)
        order = np.argsort(dist[i * T:(i + 1) * T], axis=0, kind="stable")
        unexplained = 0
        for k in np.flatnonzero(und[i]):
            a, b = order[0, k], order[1, k]
            chain = sorted(set(anc[caps[pairs[k, 0]][0]]) ^ set(anc[caps[pairs[k, 1]][0]]))
            unexplained += not np.array_equal(canon[a, chain], canon[b, chain])
        print(f"capsule winners, {key}, {c}: {int(und[i].sum())} of {len(pairs)} pairs undecided, {unexplained} of them between different poses")
        assert unexplained <= 0.02 * len(pairs), (key, c, unexplained)
        if c == "attitude":
            assert not und[i].any()
