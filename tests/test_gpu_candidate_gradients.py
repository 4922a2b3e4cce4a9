"""excitation.candidate_gradients_from_coefficients on the device: f and g are candidate_objectives_from_coefficients', the D-optimality
part candidate_dopt_gradient_from_coefficients', the collision rows candidate_collision_gradient_from_coefficients' -- bit for bit -- and
the soft-cost gradient and the position, velocity and torque rows of the constraint Jacobian (Phase C) match the Richardson differences of
tests/constraint_gradient_reference.py."""
import numpy as np
import pytest

import capsule_restatement as cr
import constraint_gradient_reference as cgr
from common import random_states
from test_capsule_gradient import shifted_capsules

pytestmark = pytest.mark.gpu
# Ten times the error the same comparison shows with NumPy rows (tests/test_constraint_gradient_host.py, 1.005e-6: the truncation of the
# forward differences at eps = 1e-7): device and NumPy round those differences differently -- 2 * 1.1e-16 |tau| / eps = 2e-9 |tau| an
# entry against slopes of the size of |tau| -- and the extrema sit at the same samples.  A wrong sign, index or block offset is off by 1.
BAR = 10.0 * cgr.MEASURED_CPU_ERROR


def _independent_columns(eng, topo, seed=1):
    import scipy.linalg as sla

    st = random_states(topo, 2000, np.random.default_rng(seed), eng.floating, use_limits=True)
    if eng.friction:
        st["sign"] = np.tanh(st["dq"] / 0.02)
    R, piv = sla.qr(eng.gram(st), pivoting=True, mode="r")
    d = np.abs(np.diag(R))
    return np.sort(piv[: int(np.sum(d > 1e-9 * d[0]))])


def _run(p, collision=None):
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine

    eng = Engine(p.topo, floating=p.floating, friction=p.friction)
    ic = _independent_columns(eng, p.topo)
    cands = [p.candidate(x) for x in p.xs]
    config = dict(p.config, collisionMode="capsule", collisionCheckStep=3, transitionDuration=3.0, transitionCollisionSamples=6)
    res = exc.candidate_gradients_from_coefficients(eng, cands, p.T, p.freq, p.x_std, ic, p.limits, p.names, config, collision=collision)
    return exc, eng, ic, cands, config, res


@pytest.mark.parametrize("make", [lambda: cgr.kuka_classic(friction=True), cgr.walkman_arm_floating_bounded], ids=["kuka-friction", "walkman-arm-fb-bounded"])
def test_gradients_of_a_batch_match_their_parts_and_the_richardson_differences(make):
    """3 candidates of 96 samples, minVelocityConstraint on.  Phase C at 10 x the CPU-measured error (BAR above); printed: the largest
    relative error of the soft-cost gradient and of a constraint row."""
    p = make()
    exc, eng, ic, cands, config, res = _run(p)
    C, n = len(cands), p.n
    obj = exc.candidate_objectives_from_coefficients(eng, cands, p.T, p.freq, p.x_std, ic, p.limits, p.names, config)
    assert np.array_equal(res["f"], obj["f"]) and np.array_equal(res["g"], obj["g"])
    assert not res["objectives"]["failed"].any()
    fd, gd = exc.candidate_dopt_gradient_from_coefficients(eng, cands, p.T, p.freq, ic, dopt_scale=res["objectives"]["dopt_scale"])
    assert np.array_equal(fd, res["objectives"]["dopt"])
    lay = res["layout"]
    assert lay == exc.constraint_layout(n, True) and res["g"].shape == (C, lay["len"])
    for k in ("wf", "q_offset", "q_range", "a", "b"):
        assert np.array_equal(res["dopt_grad"][k], gd[k]), k
        assert np.array_equal(res["obj_grad"][k], gd[k] + res["soft_grad"][k]), k
        assert res["con_grad"][k].shape == (C, lay["len"]) + gd[k].shape[1:], k
    worst_soft = worst_con = 0.0
    for c in range(C):
        J, base = p.richardson(p.xs[c])
        for k in cgr.IDX:
            assert np.array_equal(res["ag_cache"][k][c], base["idx"][k]), (c, k)
        assert np.abs(res["g"][c] - base["g"]).max() <= 1e-9 * max(np.abs(base["g"]).max(), 1.0)
        soft = exc.gradient_to_optimizer_variables({k: v[c] for k, v in res["soft_grad"].items()}, cands[c], p.nf, exact=p.bounded,
                                                   joint_limits=p.lim if p.bounded else None, q0=p.xs[c][1:1 + n] if p.bounded else None)
        rows = exc.constraint_gradient_to_optimizer_variables({k: v[c] for k, v in res["con_grad"].items()}, cands[c], p.nf, exact=p.bounded,
                                                              joint_limits=p.lim if p.bounded else None, q0=p.xs[c][1:1 + n] if p.bounded else None)
        worst_soft = max(worst_soft, cgr.relative_error(soft, 10.0 * J[0] + J[1] + 10.0 * J[2] + 10.0 * J[3]))
        worst_con = max(worst_con, cgr.relative_error(rows, J[4:]))
        assert np.abs(rows).max(axis=1).min() > 1e-3
    print(f"{p.topo.name}: relative error against Richardson differences: soft-cost gradient {worst_soft:.3e}, constraint rows {worst_con:.3e} (bar {BAR:.3e})")
    assert worst_soft <= BAR and worst_con <= BAR
    eng.close()


def test_collision_rows_are_appended_at_their_layout_offset():
    p = cgr.kuka_classic(friction=True)
    caps = shifted_capsules(p.topo, np.random.default_rng(4))
    cs = {"capsules": caps, "pairs": cr.non_neighbour_pairs(p.topo, caps)}
    exc, eng, ic, cands, config, res = _run(p, collision=cs)
    P, lay, n = len(cs["pairs"]), res["layout"], p.n
    assert lay == exc.constraint_layout(n, True, P) and lay["collision"] == 6 * n
    obj = exc.candidate_objectives_from_coefficients(eng, cands, p.T, p.freq, p.x_std, ic, p.limits, p.names, config, collision=cs)
    assert np.array_equal(res["f"], obj["f"]) and np.array_equal(res["g"], obj["g"]) and res["g"].shape[1] == lay["len"]
    coll = exc.candidate_collision_gradient_from_coefficients(eng, cands, p.T, p.freq, config, cs)
    assert np.array_equal(res["g"][:, lay["collision"]:], coll["g"])
    eng2, plain = _run(p)[1::4]
    eng2.close()
    for k, v in coll["grad"].items():
        assert np.array_equal(res["con_grad"][k][:, lay["collision"]:], v), k
        assert np.array_equal(res["con_grad"][k][:, :lay["collision"]], plain["con_grad"][k]), k
        assert np.array_equal(res["obj_grad"][k], plain["obj_grad"][k]), k
    assert np.abs(coll["grad"]["a"]).max() > 1e-3
    eng.close()


def test_refusals():
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine

    p = cgr.kuka_classic()
    eng = Engine(p.topo)
    cands = [p.candidate(x) for x in p.xs]
    for bad in ({"floatingBaseAttachment": "suspended"}, {"identifyGravityParamsOnly": 1}):
        with pytest.raises(ValueError):
            exc.candidate_gradients_from_coefficients(eng, cands, p.T, p.freq, p.x_std, np.arange(10), p.limits, p.names, dict(p.config, **bad))
    eng.close()
