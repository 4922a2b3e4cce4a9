"""fbr_candidate_extrema / Engine.candidate_extrema and the batched objective of the trajectory optimiser on the device: the per-candidate
extrema of q, |dq| and |tau| are exactly NumPy's reductions of the states and of the torques Engine.inverse_dynamics returns, on every
route (fused lane kernel, two-kernel path, link-merged model), and candidate_objectives_from_coefficients equals a restatement of
objectiveFunc (excitation/trajectoryOptimizer.py) on the host states and the oracle's torques."""
import os

import numpy as np
import pytest

from common import CONFIGS, GOLDEN, cfg_id, load_topo, random_states, random_topology
from objective_restatement import restate_from_samples

pytestmark = pytest.mark.gpu

DBL_MAX = np.finfo(np.float64).max
NAMES = ("q_min", "q_max", "dq_absmax", "tau_absmax")


def _engine_oracle(cfg, options=None):
    from flobaroid_amd._lib import Engine
    from oracle.oracle import OracleModel

    name, fl, fr, sym, grav, strb = cfg
    t = load_topo(name)
    eng = Engine(t, floating=fl, friction=fr, friction_symmetric=sym, gravity_only=grav, stribeck_velocity=strb, options=options)
    om = OracleModel(t, floating=fl, fric=fr, fric_sym=sym, grav_only=grav, stribeck=strb)
    return t, eng, om


def _states(t, cfg, S, seed):
    rng = np.random.default_rng(seed)
    st = random_states(t, S, rng, cfg[1])
    if cfg[4]:
        st["dq"][:] = 0.0
        st["ddq"][:] = 0.0
    st["sign"] = np.tanh(st["dq"] / 0.02)
    return st, rng


def _x_std(t, om, rng, cfg):
    nfric = om.P - (4 if cfg[4] else 10) * t.num_links
    return np.concatenate([t.x_std(), rng.random(max(nfric, 0) + 4 * t.num_dofs)])


def _np_extrema(q, dq, tau, C, fb):
    """NumPy's reductions, as objectiveFunc takes them (torques through np.nan_to_num, the base rows skipped)."""
    S, n = q.shape
    T = S // C
    q3, dq3 = q.reshape(C, T, n), np.abs(dq.reshape(C, T, n))
    tq = np.abs(np.nan_to_num(tau.reshape(C, T, -1)[..., fb:]))
    return {"q_min": q3.min(axis=1), "q_min_idx": q3.argmin(axis=1), "q_max": q3.max(axis=1), "q_max_idx": q3.argmax(axis=1),
            "dq_absmax": dq3.max(axis=1), "dq_absmax_idx": dq3.argmax(axis=1), "tau_absmax": tq.max(axis=1), "tau_absmax_idx": tq.argmax(axis=1)}


def _host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _assert_exact(got, want, why):
    got = _host(got)
    for k in want:
        assert got[k].shape == want[k].shape, (why, k)
        assert np.array_equal(got[k], want[k], equal_nan=not k.endswith("_idx")), (why, k)
        if k.endswith("_idx"):
            assert got[k].dtype == np.int64, (why, k)


def _to_dev(st):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in st.items()}


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_extrema_equal_numpy_on_the_engine_torques_and_match_the_oracle(cfg):
    t, eng, om = _engine_oracle(cfg)
    fb = eng.rows - eng.n
    st, rng = _states(t, cfg, 17 * 1000, 7)
    x_std = _x_std(t, om, rng, cfg)
    vel_sign = st["dq"] * 0.9
    tau_o = om.inverse_dynamics(st, x_std, st["sign"], vel_sign)
    for T in (1, 37, 64, 65, 1000):
        for C in (1, 3, 17):
            S = C * T
            sub = {k: v[:S] for k, v in st.items()}
            vs = vel_sign[:S]
            tau = eng.inverse_dynamics(sub, x_std, vel_sign=vs)
            want = _np_extrema(sub["q"], sub["dq"], tau, C, fb)
            why = (cfg_id(cfg), T, C)
            _assert_exact(eng.candidate_extrema(sub, C, x_std, vel_sign=vs), want, why + ("host",))
            wo = _np_extrema(sub["q"], sub["dq"], tau_o[:S], C, fb)
            for k in NAMES:
                assert np.abs(want[k] - wo[k]).max() <= 1e-9 * max(np.abs(wo[k]).max(), 1e-300), why + (k,)
            if T in (37, 1000):  # device states; outputs on the device and on the host
                dsub, dvs = _to_dev(sub), _to_dev({"v": vs})["v"]
                got = eng.candidate_extrema(dsub, C, x_std, vel_sign=dvs)
                assert got["q_min"].is_cuda and got["tau_absmax_idx"].is_cuda
                _assert_exact(got, want, why + ("device",))
                _assert_exact(eng.candidate_extrema(dsub, C, x_std, vel_sign=dvs, device_out=False), want, why + ("device->host",))
                _assert_exact(eng.candidate_extrema(sub, C, x_std, vel_sign=vs, device_out=True), want, why + ("host->device",))
    eng.close()


@pytest.mark.parametrize("cfg", [CONFIGS[4], CONFIGS[6], CONFIGS[7]], ids=cfg_id)
def test_each_route_equals_its_own_inverse_dynamics(cfg):
    """fused_id = 0 (the two-kernel torques + the standalone tile kernel) and link_merge = 0 (the unmerged tree) each give exactly the
    reductions of their own inverse_dynamics; the fused and the standalone routes agree exactly on q and dq."""
    results = {}
    for opts in ({}, {"fused_id": 0}, {"link_merge": 0}):
        t, eng, om = _engine_oracle(cfg, options=opts)
        fb = eng.rows - eng.n
        st, rng = _states(t, cfg, 5 * 130, 9)
        x_std = _x_std(t, om, rng, cfg)
        vs = st["dq"] * 0.7
        tau = eng.inverse_dynamics(st, x_std, vel_sign=vs)
        got = eng.candidate_extrema(st, 5, x_std, vel_sign=vs)
        _assert_exact(got, _np_extrema(st["q"], st["dq"], tau, 5, fb), (cfg_id(cfg), opts))
        results[str(opts)] = got
        eng.close()
    for k in ("q_min", "q_max", "dq_absmax"):
        for suffix in ("", "_idx"):
            assert np.array_equal(results["{}"][k + suffix], results[str({"fused_id": 0})][k + suffix]), k + suffix


def _check_own(eng, st, C, x_std, why):
    fb = eng.rows - eng.n
    tau = eng.inverse_dynamics(st, x_std)
    _assert_exact(eng.candidate_extrema(st, C, x_std), _np_extrema(st["q"], st["dq"], tau, C, fb), why)


def test_more_than_105_dof_take_the_two_kernel_route():
    from flobaroid_amd._lib import Engine

    rng = np.random.default_rng(73)
    t = random_topology(rng, 130, p_fixed=0.0, branchiness=1.0)
    assert t.num_dofs >= 110
    st = random_states(t, 3 * 70, rng, True)
    st["sign"] = np.tanh(st["dq"] / 0.02)
    for fric in (False, True):
        eng = Engine(t, floating=True, friction=fric)
        x_std = np.concatenate([t.x_std(), rng.random(4 * t.num_dofs)])
        _check_own(eng, st, 3, x_std, ("130 links", fric))
        eng.close()


@pytest.mark.parametrize("depth", [4, 5, 8, 9, 12, 13, 24, 25])
def test_joint_paths_at_the_instance_thresholds(depth):
    """A chain of `depth` joints: the register-stack instance of that depth (4, 8, 12, FBR_KINID_MAXD = 24), 25 the two-kernel path."""
    from flobaroid_amd._lib import Engine

    rng = np.random.default_rng([76, depth])
    t = random_topology(rng, depth + 1, p_fixed=0.0, branchiness=0.0, p_prismatic=0.2)
    assert t.num_dofs == depth
    floating = bool(depth % 2)
    st = random_states(t, 4 * 71, rng, floating)
    eng = Engine(t, floating=floating)
    _check_own(eng, st, 4, t.x_std(), ("depth", depth))
    eng.close()


@pytest.mark.parametrize("fused", [1, 0])
def test_70001_candidates_of_one_sample(fused):
    cfg = CONFIGS[3]
    t, eng, om = _engine_oracle(cfg, options={"fused_id": fused})
    st, rng = _states(t, cfg, 70_001, 12)
    x_std = _x_std(t, om, rng, cfg)
    got = _host(eng.candidate_extrema(st, 70_001, x_std))
    _check_own(eng, st, 70_001, x_std, ("70001", fused))
    assert np.all(got["q_min_idx"] == 0) and np.array_equal(got["q_min"], st["q"]) and np.array_equal(got["q_max"], st["q"])
    eng.close()


def test_ties_go_to_the_first_sample():
    """Every sample duplicated (2i, 2i + 1), the pairs straddling the 64-sample tiles too: every index is the even one."""
    cfg = CONFIGS[4]
    t, eng, om = _engine_oracle(cfg)
    fb = eng.rows - eng.n
    C, T = 3, 130
    st, rng = _states(t, cfg, C * T // 2, 21)
    st = {k: np.repeat(v, 2, axis=0) for k, v in st.items()}
    x_std = _x_std(t, om, rng, cfg)
    vs = st["dq"].copy()
    tau = eng.inverse_dynamics(st, x_std, vel_sign=vs)
    assert np.array_equal(tau[0::2], tau[1::2])
    got = _host(eng.candidate_extrema(st, C, x_std, vel_sign=vs))
    _assert_exact(got, _np_extrema(st["q"], st["dq"], tau, C, fb), "ties")
    for k in NAMES:
        assert np.all(got[k + "_idx"] % 2 == 0), k
    eng.close()


def test_nan_and_inf_follow_numpy():
    """A NaN in one dq: that joint's |dq| maximum is NaN at that sample, the other joints are untouched; the sample's torques are NaN and
    count as 0.  A NaN in q likewise for min / max q.  An inf torque counts as DBL_MAX."""
    cfg = CONFIGS[2]  # kuka_lwr4, fixed base, no friction
    t, eng, om = _engine_oracle(cfg)
    fb = eng.rows - eng.n
    C, T = 2, 150
    st, rng = _states(t, cfg, C * T, 31)
    x_std = t.x_std()
    st["dq"][T + 100, 3] = np.nan  # candidate 1, sample 100, joint 3
    st["q"][70, 5] = np.nan        # candidate 0, sample 70, joint 5
    tau = eng.inverse_dynamics(st, x_std)
    assert np.isnan(tau[T + 100, fb:]).any()
    got = _host(eng.candidate_extrema(st, C, x_std))
    _assert_exact(got, _np_extrema(st["q"], st["dq"], tau, C, fb), "nan")
    assert np.isnan(got["dq_absmax"][1, 3]) and got["dq_absmax_idx"][1, 3] == 100
    assert np.isfinite(np.delete(got["dq_absmax"][1], 3)).all() and np.isfinite(got["dq_absmax"][0]).all()
    assert np.isnan(got["q_min"][0, 5]) and np.isnan(got["q_max"][0, 5]) and got["q_min_idx"][0, 5] == got["q_max_idx"][0, 5] == 70
    assert np.isfinite(got["tau_absmax"]).all()
    eng.close()
    # inf: a viscous friction coefficient of 1e308 on joint 2 overflows that joint's torque wherever |dq_2| > 1.8 (+-inf, no NaN)
    t, eng, om = _engine_oracle(CONFIGS[3])
    st2, rng = _states(t, CONFIGS[3], C * T, 32)
    x2 = _x_std(t, om, rng, CONFIGS[3])
    x2[10 * t.num_links + t.num_dofs + 2] = 1e308
    tau2 = eng.inverse_dynamics(st2, x2)
    assert np.isinf(tau2[:T, 2]).any() and not np.isnan(tau2).any()
    got2 = _host(eng.candidate_extrema(st2, C, x2))
    _assert_exact(got2, _np_extrema(st2["q"], st2["dq"], tau2, C, 0), "inf")
    first = int(np.flatnonzero(np.isinf(tau2[:T, 2]))[0])
    assert got2["tau_absmax"][0, 2] == DBL_MAX and got2["tau_absmax_idx"][0, 2] == first
    eng.close()


def test_errors_and_determinism():
    from flobaroid_amd._lib import FbrError

    cfg = CONFIGS[4]  # Stribeck
    t, eng, om = _engine_oracle(cfg)
    st, rng = _states(t, cfg, 6 * 50, 41)
    x_std = _x_std(t, om, rng, cfg)
    vs = st["dq"]
    for bad in (0, -2, 7):
        with pytest.raises(FbrError):
            eng.candidate_extrema(st, bad, x_std, vel_sign=vs)
    with pytest.raises(FbrError):
        eng.candidate_extrema(st, 6, x_std)  # Stribeck without vel_sign
    with pytest.raises(FbrError):
        eng.candidate_extrema(st, 6, x_std[:5], vel_sign=vs)
    with pytest.raises(FbrError):
        eng.candidate_extrema({k: v[:0] for k, v in st.items()}, 1, x_std, vel_sign=vs[:0])
    first = _host(eng.candidate_extrema(_to_dev(st), 6, x_std, vel_sign=_to_dev({"v": vs})["v"]))
    for _ in range(4):
        again = _host(eng.candidate_extrema(_to_dev(st), 6, x_std, vel_sign=_to_dev({"v": vs})["v"]))
        for k in first:
            assert first[k].tobytes() == again[k].tobytes(), k
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end: Fourier coefficients -> objective, the torques never leaving the device
# ------------------------------------------------------------------------------------------------------------------------------------
def _fixture():
    return dict(np.load(os.path.join(GOLDEN, "ref_trajectories.npz"), allow_pickle=False))


def _candidate(fx, c, mode):
    from flobaroid_amd import excitation as exc

    n = int(fx["num_dofs"])
    nf = fx[f"c{c}_nf"]
    a = [fx[f"c{c}_a"][j, : nf[j]] for j in range(n)]
    b = [fx[f"c{c}_b"][j, : nf[j]] for j in range(n)]
    lim = [tuple(l) for l in fx["joint_limits"]] if mode == "bounded" else None
    return exc.fourier_coefficients(a, b, fx[f"c{c}_q0"], nf, float(fx[f"c{c}_wf"]), joint_limits=lim)


@pytest.mark.parametrize("mode", ["classic", "bounded"])
def test_objectives_from_coefficients_match_the_restatement(mode, monkeypatch):
    import scipy.linalg as sla

    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from oracle.oracle import OracleModel

    fx = _fixture()
    t = load_topo("kuka_lwr4")
    eng = Engine(t)
    om = OracleModel(t)
    C = int(fx["num_cases"])
    T = min(fx[f"c{c}_{mode}_positions"].shape[0] for c in range(C))
    freq = float(fx["freq"])
    cands = [_candidate(fx, c, mode) for c in range(C)]
    x_std = t.x_std()
    rng = np.random.default_rng(1)
    ic = np.sort(sla.qr(eng.gram(random_states(t, 2000, rng, False, use_limits=True)), pivoting=True, mode="r")[1][:43])
    names = list(t.dof_names)
    config = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0,
              "ovrPosLimit": {names[2]: [-100.0, 100.0]}}

    def _boom(*a, **k):
        raise AssertionError("the torques must not leave the device")

    monkeypatch.setattr(Engine, "inverse_dynamics", _boom)
    out = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, x_std, ic, t.limits, names, config)
    monkeypatch.undo()

    nlds, refs = [], []
    for c in range(C):
        host = {k: fx[f"c{c}_{mode}_{r}"][:T] for k, r in (("q", "positions"), ("dq", "velocities"), ("ddq", "accelerations"))}
        Yb = om.regressor(host)[:, ic]
        ev = np.linalg.eigvalsh(Yb.T @ Yb)
        delta = 1e-4 * max(ev[-1], 1e-30)
        nlds.append(-np.sum(np.log(np.maximum(ev + delta, 1e-300))))
        assert out["n_observable"][c] == int(np.sum(ev > delta))
        refs.append((host, om.inverse_dynamics(host, x_std)))
    scale = 10.0 / max(abs(nlds[0]), 1.0)
    assert abs(out["dopt_scale"] - scale) <= 1e-9 * scale
    for c, (host, tau_o) in enumerate(refs):
        ref = restate_from_samples(nlds[c], host["q"], host["dq"], tau_o, 0, t.limits, names, config, scale)
        assert np.abs(out["g"][c] - ref["g"]).max() <= 1e-9 * max(np.abs(ref["g"]).max(), 1.0), c
        for k in ("f", "dopt", "f1", "f2", "f3", "f4"):
            assert abs(out[k][c] - ref[k]) <= 1e-9 * max(abs(ref[k]), 1.0), (c, k, out[k][c], ref[k])
        assert not out["failed"][c]
        for k, v in ref["idx"].items():
            assert np.array_equal(out["ag_cache"][k][c], v), (c, k)
    eng.close()
