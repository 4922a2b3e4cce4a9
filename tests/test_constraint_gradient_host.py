"""excitation.constraint_gradients_from_rows (Phase C of the analytical gradient: soft-cost gradients and the position, velocity and torque
rows of the constraint Jacobian) on the host: fed with rows computed in NumPy -- np_dynamics torques under the same forward-difference step,
the series Jacobian of fourier_gradient_restatement -- every soft-cost gradient and every constraint row, mapped to the optimiser's
variables, against Richardson-extrapolated central differences of objective_restatement.restate_from_samples
(tests/constraint_gradient_reference.py)."""
import numpy as np
import pytest

import constraint_gradient_reference as cgr

EPS = 1e-7
# What separates the two sides is the truncation of the forward differences behind the torque rows, eps / 2 |d2 tau| / |d tau| per entry:
# 1e-7 / 2 times a curvature-to-slope ratio of the torques that stays below a hundred for these arms (sines and cosines of the joint angles,
# squares of velocities of a few rad/s) -- 5e-6 at the outside; the Richardson differences themselves (h = 1e-5: truncation ~ h^4, rounding
# ~ 1e-16 / h) and the analytic position and velocity rows sit at 1e-10.  A wrong sign, sample index or block offset is off by the size
# of the row, 1.
BOUND = 1e-5


@pytest.mark.parametrize("make", [cgr.kuka_classic, cgr.three_links_floating_bounded], ids=["kuka-classic", "threeLinks-floating-bounded"])
def test_phase_c_matches_richardson_differences(make):
    """KUKA classic (3 candidates of 96 samples, minVelocityConstraint on) and threeLinks floating bounded.  Measured: the largest relative
    error (constraint_gradient_reference.relative_error) is 1.005e-6 on KUKA and 3.4e-7 on threeLinks -- the forward differences' truncation;
    constraint_gradient_reference.MEASURED_CPU_ERROR records it for the device comparison."""
    from flobaroid_amd import excitation as exc

    p = make()
    C = len(p.xs)
    cands = [p.candidate(x) for x in p.xs]
    evs = [p.evaluate(x) for x in p.xs]
    ag = p.ag_cache(evs)
    assert (ag["f3"] > 0).any() and (ag["f3"] == 0).any(), "no candidate on either side of the torque-utilisation target: change the seed"
    assert np.all(ag["util_std"] > 0) and np.all(ag["util_mean"] > 0), "change the seed"
    vt = p.config["trajectoryTargetVelocity"]
    assert (ag["vel_absmax"] < vt).any() and (ag["vel_absmax"] >= vt).any(), "no joints on both sides of the target velocity: change the seed"
    jac = p.torque_jacobians(evs, ag, EPS)
    vel = np.stack([e["dq"][ag["vel_absmax_idx"][c], np.arange(p.n)] for c, e in enumerate(evs)])
    out = exc.constraint_gradients_from_rows(ag, jac, vel, p.chain(cands), p.limits, p.names, p.config)
    lay = exc.constraint_layout(p.n, bool(p.config.get("minVelocityConstraint")))
    assert out["con_grad"].shape[:2] == (C, lay["len"]) and out["obj_grad"].shape == out["df1"].shape
    assert np.array_equal(out["obj_grad"], 10.0 * out["df1"] + 10.0 * out["df3"] + out["df2"] + 10.0 * out["df4"])
    worst = 0.0
    for c in range(C):
        J, base = p.richardson(p.xs[c])  # (asserts that the four index arrays are the same at every stencil point)
        for k in cgr.IDX:
            assert np.array_equal(base["idx"][k], ag[k][c])
        got = cgr.assembled(p, out, c)
        assert got.shape == J.shape
        err = cgr.relative_error(got, J)
        worst = max(worst, err)
        assert np.abs(J[4:]).max(axis=1).min() > 1e-3  # no constraint row is empty
        if ag["f3"][c] == 0:
            assert np.all(got[2] == 0.0) and np.all(J[2] == 0.0)
        assert err <= BOUND, (c, err)
    print(f"{p.topo.name}: largest relative error of a soft-cost gradient or constraint row against Richardson differences: {worst:.3e}")


def test_conditions_and_layout_follow_the_reference():
    """f1 off where util_std == 0, f4 off without a target velocity, the minimum-velocity block present only when configured, torch in, torch out"""
    import torch

    from flobaroid_amd import excitation as exc

    p = cgr.three_links_floating_bounded()
    cands = [p.candidate(x) for x in p.xs]
    evs = [p.evaluate(x) for x in p.xs]
    ag = p.ag_cache(evs)
    jac = p.torque_jacobians(evs, ag, EPS)
    vel = np.stack([e["dq"][ag["vel_absmax_idx"][c], np.arange(p.n)] for c, e in enumerate(evs)])
    chain = p.chain(cands)
    ref = exc.constraint_gradients_from_rows(ag, jac, vel, chain, p.limits, p.names, p.config)
    n = p.n
    flat = dict(ag, util_std=np.zeros(len(p.xs)))
    assert np.all(exc.constraint_gradients_from_rows(flat, jac, vel, chain, p.limits, p.names, p.config)["df1"] == 0.0)
    cfg = dict(p.config, trajectoryTargetVelocity=0.0, minVelocityConstraint=True, minVelocityPercentage=0.1)
    out = exc.constraint_gradients_from_rows(ag, jac, vel, chain, p.limits, p.names, cfg)
    assert np.all(out["df4"] == 0.0) and out["con_grad"].shape[1] == 6 * n
    lay = exc.constraint_layout(n, True)
    assert np.array_equal(out["con_grad"][:, lay["min_vel"]:lay["min_vel"] + n], -out["con_grad"][:, lay["vel"]:lay["vel"] + n])
    assert np.array_equal(out["con_grad"][:, lay["min_torque_util"]:], -out["con_grad"][:, lay["torque"]:lay["torque"] + n])
    assert np.array_equal(out["con_grad"][:, :4 * n], ref["con_grad"][:, :4 * n])
    tj = {k: torch.from_numpy(v) for k, v in jac.items()}
    tchain = lambda s, a, b, c: torch.from_numpy(chain(s.numpy(), a.numpy(), b.numpy(), c.numpy()))  # noqa: E731
    tout = exc.constraint_gradients_from_rows(ag, tj, vel, tchain, p.limits, p.names, p.config)
    for k in ("obj_grad", "con_grad"):
        assert isinstance(tout[k], torch.Tensor) and np.abs(tout[k].numpy() - ref[k]).max() <= 1e-14 * np.abs(ref[k]).max()
    with pytest.raises(ValueError):
        exc.constraint_gradients_from_rows(ag, jac, vel, chain, p.limits, p.names, dict(p.config, floatingBaseAttachment="suspended"))
