"""excitation.constraint_gradients_from_rows(..., suspended=) on the host, fed with NumPy rows under both rules of the suspended base
(tests/suspended_gradient_reference.py): ``"held"`` -- sweeps at the swung base -- against the Richardson differences of the frozen-base
objective; ``"identity"`` -- sweeps at the rest base, signs and peak samples from the swung torques -- against sign(tau_swung) times the
Richardson derivative of the rest-base torque at those samples.  Also rest_base_states and the refusals that need no engine."""
import numpy as np
import pytest

import constraint_gradient_reference as cgr
import suspended_gradient_reference as sgr

EPS = 1e-7
ARM = dict(seed=0, target_util=0.1)
THREE = dict(seed=2)
PROBLEMS = [lambda: sgr.walkman_arm_suspended(**ARM), lambda: sgr.three_links_suspended(**THREE)]
IDS = ["walkman-arm-LShy", "threeLinks-last-link"]
_cache = {}


def solved(i):
    """problem i, its candidates and per candidate (J_held, evaluation, base arrays), computed once and left unchanged"""
    if i not in _cache:
        p = PROBLEMS[i]()
        _cache[i] = (p, [p.candidate(x) for x in p.xs], [p.richardson_held(x) for x in p.xs])
    return _cache[i]


def rows(p, cands, sol, rest_base):
    from flobaroid_amd import excitation as exc

    evs, bases = [s[1] for s in sol], [s[2] for s in sol]
    ag = p.ag_cache(evs)
    jac = p.torque_jacobians_at(evs, bases, ag, EPS, rest_base)
    vel = np.stack([e["dq"][ag["vel_absmax_idx"][c], np.arange(p.n)] for c, e in enumerate(evs)])
    return ag, jac, exc.constraint_gradients_from_rows(ag, jac, vel, p.chain(cands), p.limits, p.names, p.config, suspended=p.spec)


@pytest.mark.parametrize("i", [0, 1], ids=IDS)
def test_both_rules_match_their_yardsticks(i):
    """3 candidates each.  Measured (printed): the largest relative error of a soft-cost gradient or constraint row, per rule; the constants
    of suspended_gradient_reference record the larger of the two problems and this test holds the figures within twice those."""
    from flobaroid_amd import excitation as exc

    p, cands, sol = solved(i)
    C, n = len(cands), p.n
    assert max(np.abs(s[2]["rpy"]).max() for s in sol) > 1e-3, "the base does not swing"
    ag, jac_h, held = rows(p, cands, sol, False)
    _, jac_i, ident = rows(p, cands, sol, True)
    assert (ag["f3"] > 0).any() and (ag["f3"] == 0).any(), "no candidate on either side of the torque-utilisation target: change the seed"
    assert np.all(ag["util_std"] > 0) and np.all(ag["util_mean"] > 0)
    assert np.array_equal(jac_h["tau"], jac_i["tau"])  # tau is the swung torque under both rules
    lay = exc.constraint_layout(n, bool(p.config.get("minVelocityConstraint")))
    assert held["con_grad"].shape[:2] == (C, lay["len"])
    # the position and velocity rows do not see the rule
    pv = np.concatenate([np.arange(lay[b], lay[b] + n) for b in ("pos_lower", "pos_upper", "vel", "min_vel") if b in lay])
    assert np.array_equal(held["con_grad"][:, pv], ident["con_grad"][:, pv])
    assert np.array_equal(held["df2"], ident["df2"]) and np.array_equal(held["df4"], ident["df4"])
    worst = {"held": 0.0, "identity": 0.0}
    differ = 0.0
    for c in range(C):
        J, ev, base = sol[c]
        for k in cgr.IDX:
            assert np.array_equal(ev["idx"][k], ag[k][c])
        assert np.abs(J[4:]).max(axis=1).min() > 1e-3  # no constraint row is empty
        got = cgr.assembled(p, held, c)
        worst["held"] = max(worst["held"], cgr.relative_error(got, J))
        Ji = p.identity_jacobian(p.xs[c], J, ev)
        goti = cgr.assembled(p, ident, c)
        live = np.r_[0, 2, 4 + lay["torque"]:4 + lay["torque"] + n, 4 + lay["min_torque_util"]:4 + lay["min_torque_util"] + n]
        worst["identity"] = max(worst["identity"], cgr.relative_error(goti[live], Ji[live]))
        differ = max(differ, cgr.relative_error(goti[live], J[live]))
        if ag["f3"][c] == 0:
            assert np.all(goti[2] == 0.0) and np.all(got[2] == 0.0)
    print(f"{IDS[i]}: largest relative error held {worst['held']:.3e}, identity {worst['identity']:.3e}; the two rules differ by {differ:.3e}")
    assert differ > 1e-2, "the rules cannot be told apart on this problem"
    assert worst["held"] <= 2.0 * sgr.MEASURED_CPU_ERROR_HELD and worst["identity"] <= 2.0 * sgr.MEASURED_CPU_ERROR_IDENTITY


def test_a_torque_row_carries_the_swung_sign():
    """On the arm some joints' rest-base torque at the sample of their (swung) torque peak has the opposite sign of the swung torque
    (asserted); the row of the reference's rule is sign(tau_swung) d tau_rest, not sign(tau_rest) d tau_rest."""
    from flobaroid_amd import excitation as exc

    p, cands, sol = solved(0)
    ag, jac, ident = rows(p, cands, sol, True)
    lay = exc.constraint_layout(p.n, True)
    found = 0
    for c, (J, ev, base) in enumerate(sol):
        s = ag["torque_absmax_idx"][c]
        rest = p.torques_at(ev["q"], ev["dq"], ev["ddq"], p.rest(p.T))[s, p.fb + np.arange(p.n)]
        swung = jac["tau"][c]
        d_rest = p.richardson_rows_identity(p.xs[c], s)
        got = p.to_variables(np.asarray(ident["con_grad"][c, lay["torque"]:lay["torque"] + p.n]), c)
        for j in np.flatnonzero(np.sign(rest) * np.sign(swung) < 0):
            found += 1
            scale = np.abs(d_rest[j]).max()
            assert scale > 1e-3
            assert np.abs(got[j] - np.sign(swung[j]) * d_rest[j]).max() <= 1e-4 * scale
            assert np.abs(got[j] - np.sign(rest[j]) * d_rest[j]).max() >= scale
    assert found >= 1, "no joint with opposite signs at its peak: change the seed"


def test_rest_base_states():
    import torch

    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(0)
    st = {"q": rng.standard_normal((5, 2)), "dq": rng.standard_normal((5, 2)), "ddq": rng.standard_normal((5, 2)), "sign": rng.standard_normal((5, 2)),
          "rpy": rng.standard_normal((5, 3)), "base_vel": rng.standard_normal((5, 6)), "base_acc": rng.standard_normal((5, 6)),
          "base_position": rng.standard_normal((5, 3))}
    keep = {k: v.copy() for k, v in st.items()}
    for kind in (lambda a: a, torch.from_numpy):
        src = {k: kind(v) for k, v in st.items()}
        out = exc.rest_base_states(src)
        assert set(out) == set(src)
        for k in ("q", "dq", "ddq", "sign", "base_position"):
            assert out[k] is src[k], k
        for k in ("rpy", "base_vel", "base_acc"):
            assert type(out[k]) is type(src[k]) and tuple(out[k].shape) == tuple(src[k].shape) and out[k].dtype == src[k].dtype
            assert not np.asarray(out[k]).any() and out[k] is not src[k], k
    assert all(np.array_equal(st[k], keep[k]) for k in st)  # the input's base arrays are left alone
    alias = exc.rest_base_states({"q": st["q"], "base_rpy": st["rpy"], "base_velocity": st["base_vel"], "base_acceleration": st["base_acc"]})
    assert not any(alias[k].any() for k in ("base_rpy", "base_velocity", "base_acceleration"))
    assert set(exc.rest_base_states({"q": st["q"]})) == {"q"}  # a fixed base has nothing to zero


def test_refusals_without_an_engine():
    from flobaroid_amd import excitation as exc

    p, cands, sol = solved(1)
    evs, bases = [s[1] for s in sol], [s[2] for s in sol]
    ag = p.ag_cache(evs)
    jac = p.torque_jacobians_at(evs, bases, ag, EPS, True)
    vel = np.stack([e["dq"][ag["vel_absmax_idx"][c], np.arange(p.n)] for c, e in enumerate(evs)])
    args = (ag, jac, vel, p.chain(cands), p.limits, p.names)
    with pytest.raises(ValueError, match="suspended"):
        exc.constraint_gradients_from_rows(*args, p.config)  # the configuration without suspended=
    with pytest.raises(ValueError, match="identifyGravityParamsOnly"):
        exc.constraint_gradients_from_rows(*args, dict(p.config, identifyGravityParamsOnly=1), suspended=p.spec)
    with pytest.raises(ValueError, match="unknown keys"):
        exc.constraint_gradients_from_rows(*args, p.config, suspended=dict(p.spec, dampling=1.0))
    plain = dict(p.config, floatingBaseAttachment="fixed")
    a, b = exc.constraint_gradients_from_rows(*args, plain), exc.constraint_gradients_from_rows(*args, plain, suspended=None)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for rule in ("Identity", "rest", None):
        with pytest.raises(ValueError, match="suspended_base"):
            exc._suspended_rule(p.spec, rule)
    with pytest.raises(ValueError, match="without suspended="):
        exc._suspended_rule(None, "held")
    assert exc._suspended_rule(p.spec, "identity") and not exc._suspended_rule(p.spec, "held") and not exc._suspended_rule(None, "identity")
