"""The batched objective of the trajectory optimiser on the host (excitation.objectives_from_extrema): f, g and the soft costs of
objectiveFunc (excitation/trajectoryOptimizer.py) from per-candidate extrema, against a per-candidate restatement of the reference's rules.
No GPU: the extrema are synthetic."""
import numpy as np
import pytest

from objective_restatement import restate_objective


def _limits(n, rng):
    names = [f"j{i}" for i in range(n)]
    lo = -1.0 - rng.random(n)
    hi = 1.0 + rng.random(n)
    return names, {j: {"lower": lo[i], "upper": hi[i], "velocity": 1.0 + 2 * rng.random(), "torque": 10.0 + 50 * rng.random()}
                   for i, j in enumerate(names)}


def _extrema(C, n, rng):
    qmin = -1.5 * rng.random((C, n))
    ext = {"q_min": qmin, "q_max": qmin + 2.5 * rng.random((C, n)), "dq_absmax": 3 * rng.random((C, n)),
           "tau_absmax": 60 * rng.random((C, n))}
    for k in list(ext):
        ext[k + "_idx"] = rng.integers(0, 100, (C, n))
    return ext


def _check(out, C, n, nld, nobs, ext, limits, names, config, dopt_scale):
    for c in range(C):
        ref = restate_objective(nld[c], {k: v[c] for k, v in ext.items()}, limits, names, config,
                                dopt_scale if dopt_scale is not None else 10.0 / max(abs(nld[0]), 1.0))
        assert out["g"][c].shape == ref["g"].shape
        np.testing.assert_allclose(out["g"][c], ref["g"], rtol=1e-12, atol=1e-12)
        for k in ("f", "dopt", "f1", "f2", "f3", "f4"):
            if not np.isfinite(ref[k]):  # (a NaN position reaches f through the position range, in the reference as well)
                assert np.array_equal(out[k][c], ref[k], equal_nan=True), (k, c)
                continue
            assert abs(out[k][c] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), (k, c, out[k][c], ref[k])
        assert bool(out["failed"][c]) == ref["failed"]
        assert out["n_observable"][c] == nobs[c]
    for a, b in (("torque_absmax_idx", "tau_absmax_idx"), ("pos_min_idx", "q_min_idx"), ("pos_max_idx", "q_max_idx"),
                 ("vel_absmax_idx", "dq_absmax_idx")):
        assert np.array_equal(out["ag_cache"][a], ext[b])


@pytest.mark.parametrize("minvel", [False, True])
@pytest.mark.parametrize("ovr", [False, True])
def test_objectives_match_the_restatement(minvel, ovr):
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng([11, minvel, ovr])
    C, n = 9, 7
    names, limits = _limits(n, rng)
    ext = _extrema(C, n, rng)
    nld = -50 - 100 * rng.random(C)
    nobs = rng.integers(10, 40, C)
    config = {"minVelocityConstraint": minvel, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.5 if minvel else 0.0}
    if ovr:
        config["ovrPosLimit"] = {names[1]: [-30.0, 45.0], names[4]: [-10.0, 10.0]}
    out = exc.objectives_from_extrema(nld, nobs, ext, limits, names, config, None)
    _check(out, C, n, nld, nobs, ext, limits, names, config, None)
    assert out["dopt_scale"] == 10.0 / max(abs(nld[0]), 1.0)


def test_g_layout_and_length():
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(3)
    n = 5
    names, limits = _limits(n, rng)
    ext = _extrema(2, n, rng)
    for minvel, blocks in ((False, 5), (True, 6)):
        lay = exc.constraint_layout(n, minvel)
        assert lay["len"] == blocks * n
        out = exc.objectives_from_extrema(np.array([-80.0, -90.0]), np.array([3, 4]), ext, limits, names,
                                          {"minVelocityConstraint": minvel, "minVelocityPercentage": 0.2}, 0.1)
        assert out["g"].shape == (2, blocks * n)
        lo = np.array([limits[j]["lower"] for j in names])
        tl = np.array([limits[j]["torque"] for j in names])
        vl = np.array([limits[j]["velocity"] for j in names])
        assert np.allclose(out["g"][:, lay["pos_lower"]:lay["pos_lower"] + n], lo - ext["q_min"])
        assert np.allclose(out["g"][:, lay["torque"]:lay["torque"] + n], ext["tau_absmax"] - tl)
        assert np.allclose(out["g"][:, lay["min_torque_util"]:], tl * 0.02 - ext["tau_absmax"])
        if minvel:
            assert lay["min_vel"] == 4 * n and np.allclose(out["g"][:, 4 * n:5 * n], vl * 0.2 - ext["dq_absmax"])


def test_nan_in_g_becomes_10_and_a_non_finite_dopt_fails_the_candidate():
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(5)
    C, n = 4, 6
    names, limits = _limits(n, rng)
    ext = _extrema(C, n, rng)
    ext["q_min"][1, 2] = np.nan      # a NaN position reaches the lower-limit constraint
    ext["dq_absmax"][2, 0] = np.nan  # and a NaN velocity the velocity constraint
    nld = np.array([-70.0, -60.0, np.inf, np.nan])
    config = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1}
    out = exc.objectives_from_extrema(nld, np.arange(C), ext, limits, names, config, 0.2)
    assert not np.isnan(out["g"]).any()
    assert out["g"][1, 2] == 10.0 and out["g"][2, 2 * n] == 10.0 and out["g"][2, 4 * n] == 10.0
    assert list(out["failed"]) == [False, False, True, True]
    _check(out, C, n, nld, np.arange(C), ext, limits, names, config, 0.2)
    assert np.isnan(out["f"][1]) and np.all(out["f"][2:] >= 100.0)


def test_explicit_dopt_scale_against_the_default():
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(8)
    C, n = 3, 4
    names, limits = _limits(n, rng)
    ext = _extrema(C, n, rng)
    nld = np.array([-0.5, -40.0, -80.0])  # |neg_log_det[0]| < 1: the default scale is 10
    a = exc.objectives_from_extrema(nld, np.ones(C), ext, limits, names, {}, None)
    b = exc.objectives_from_extrema(nld, np.ones(C), ext, limits, names, {}, 10.0)
    c = exc.objectives_from_extrema(nld, np.ones(C), ext, limits, names, {}, 0.25)
    assert a["dopt_scale"] == 10.0 and np.array_equal(a["f"], b["f"])
    assert np.allclose(c["f"] - a["f"], nld * (0.25 - 10.0))
    _check(c, C, n, nld, np.ones(C), ext, limits, names, {}, 0.25)


@pytest.mark.parametrize("config", [{"floatingBaseAttachment": "suspended"}, {"identifyGravityParamsOnly": 1}])
def test_unsupported_configurations_raise(config):
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(1)
    names, limits = _limits(3, rng)
    with pytest.raises(ValueError):
        exc.objectives_from_extrema(np.array([-1.0]), np.array([1]), _extrema(1, 3, rng), limits, names, config, None)
    with pytest.raises(ValueError):
        exc.candidate_objectives(None, {}, 1, [0], np.zeros(30), limits, names, config)
    with pytest.raises(ValueError):
        exc.candidate_objectives_from_coefficients(None, [], 10, 100.0, np.zeros(30), [0], limits, names, config)
