"""fbr_torque_row_sweep / Engine.torque_row_sweep: every entry is the requested joint row of the inverse dynamics at the explicitly
perturbed state -- against the CPU oracle at the bar of test_gpu_parity.py (1e-11 max|tau|) and against the engine's own
inverse_dynamics on the same perturbed states at 1e-13 max|tau|, on the fused lane route, the two-kernel route (fused_id = 0) and the
unmerged tree (link_merge = 0); the same bits on every run; indices out of range are refused."""
import numpy as np
import pytest

from common import load_topo, random_states, random_topology

pytestmark = pytest.mark.gpu
EPS = 1e-7

# name -> (floating, friction, stribeck)
ROBOTS = {"threeLinks": (0, 0, 0.0), "kuka_lwr4-fr": (0, 1, 0.0), "kuka_lwr4-stribeck": (0, 1, 0.05), "walkman_left_arm": (1, 1, 0.0),
          "random": (1, 0, 0.0)}


def _topo(name):
    if name == "random":
        return random_topology(np.random.default_rng(17), 17, p_fixed=0.25, branchiness=0.5, p_prismatic=0.3)
    return load_topo(name.split("-")[0])


def _engine(name, t, options=None):
    from flobaroid_amd._lib import Engine

    fl, fr, strb = ROBOTS[name]
    return Engine(t, floating=bool(fl), friction=bool(fr), stribeck_velocity=strb, options=options)


def _oracle(name, t):
    from oracle.oracle import OracleModel

    fl, fr, strb = ROBOTS[name]
    return OracleModel(t, floating=bool(fl), fric=bool(fr), stribeck=strb)


def _cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(name, t, C, T, seed):
    rng = np.random.default_rng(seed)
    st = random_states(t, C * T, rng, bool(ROBOTS[name][0]))
    st["sign"] = np.tanh(st["dq"] / 0.02)
    vs = st["dq"] * 0.9 if ROBOTS[name][2] > 0 else None
    x_std = np.concatenate([t.x_std(), rng.random(8 * t.num_dofs)])
    return st, vs, x_std, rng


def _perturbed(st, vs, T, sample, joint, n):
    """The states the sweep evaluates, written out: per item (c, r) the sample's state and its 3 n copies with +EPS on one entry of q / dq /
    ddq; the sign series, vel_sign and the base state repeated.  Returns (states, vel_sign, row offset of every evaluation's joint)."""
    C, R = sample.shape
    nper = 1 + 3 * n
    s = (np.arange(C)[:, None] * T + sample).reshape(-1)
    rep = {k: np.repeat(v[s], nper, axis=0) for k, v in st.items()}
    for i in range(C * R):
        for kind, key in enumerate(("q", "dq", "ddq")):
            for d in range(n):
                rep[key][i * nper + 1 + kind * n + d, d] += EPS
    jn = (np.tile(np.arange(n), (C, 1)) if joint is None else joint).reshape(-1)
    return rep, (None if vs is None else np.repeat(vs[s], nper, axis=0)), np.repeat(jn, nper)


def _shapes(name, n, rng):
    """(C, T, sample, joint): joint NULL, one explicit row, n + 2 rows with repeats; samples 0, T - 1 and interior ones"""
    out = []
    for C, T in ((1, 1), (3, 7), (17, 65)):
        for R, explicit in ((n, False), (1, True), (n + 2, True)):
            sample = rng.integers(0, T, (C, R)).astype(np.int64)
            sample[0, 0], sample[-1, -1] = 0, T - 1
            if R > 2:
                sample[0, 1] = T // 2
            joint = None
            if explicit:
                joint = rng.integers(0, n, (C, R)).astype(np.int32)
                joint[0, 0], joint[-1, -1] = n - 1, 0
                if R > 2:
                    joint[:, 1] = joint[:, 2]  # a repeat
            out.append((C, T, sample, joint))
    if name == "kuka_lwr4-fr":  # 32 items of 22 evaluations: 704 = 11 full waves
        out.append((32, 3, rng.integers(0, 3, (32, 1)).astype(np.int64), rng.integers(0, n, (32, 1)).astype(np.int32)))
    return out


@pytest.mark.parametrize("name", list(ROBOTS))
def test_sweep_rows_match_the_oracle_and_the_engine_on_every_route(name):
    t = _topo(name)
    n = t.num_dofs
    om = _oracle(name, t)
    fb = 6 if ROBOTS[name][0] else 0
    shapes = _shapes(name, n, np.random.default_rng(5))
    refs = []
    for C, T, sample, joint in shapes:
        st, vs, x_std, _ = _batch(name, t, C, T, 100 + C)
        pert, pvs, jn = _perturbed(st, vs, T, sample, joint, n)
        tau_o = om.inverse_dynamics(pert, x_std, pert["sign"], pvs)
        refs.append((st, vs, x_std, pert, pvs, jn, tau_o))
    worst_o = worst_e = 0.0
    for opts in ({}, {"fused_id": 0}, {"link_merge": 0}):
        eng = _engine(name, t, opts)
        bit_equal = True
        for (C, T, sample, joint), (st, vs, x_std, pert, pvs, jn, tau_o) in zip(shapes, refs):
            why = (name, opts, C, T, sample.shape[1], joint is None)
            got = eng.torque_row_sweep(st, C, sample, x_std, EPS, joint=joint, vel_sign=vs)
            assert isinstance(got, np.ndarray) and got.shape == (C, sample.shape[1], 1 + 3 * n), why
            rows = np.arange(jn.size)
            want_o = tau_o[rows, fb + jn].reshape(got.shape)
            err_o = np.abs(got - want_o).max() / np.abs(tau_o).max()
            tau_e = eng.inverse_dynamics(pert, x_std, vel_sign=pvs)
            want_e = tau_e[rows, fb + jn].reshape(got.shape)
            err_e = np.abs(got - want_e).max() / np.abs(tau_e).max()
            worst_o, worst_e = max(worst_o, err_o), max(worst_e, err_e)
            bit_equal &= np.array_equal(got, want_e)
            assert err_o <= 1e-11, why + (err_o,)
            assert err_e <= 1e-13, why + (err_e,)
            assert np.array_equal(got, eng.torque_row_sweep(st, C, sample, x_std, EPS, joint=joint, vel_sign=vs)), why  # the same bits again
            if C == 3:  # device inputs, device output; and a device call that returns to the host
                dst = {k: _cuda(v) for k, v in st.items()}
                dev = eng.torque_row_sweep(dst, C, _cuda(sample), x_std, EPS, joint=_cuda(joint), vel_sign=_cuda(vs))
                assert hasattr(dev, "cpu") and np.array_equal(dev.cpu().numpy(), got), why
                back = eng.torque_row_sweep(dst, C, sample, x_std, EPS, joint=joint, vel_sign=_cuda(vs), device_out=False)
                assert isinstance(back, np.ndarray) and np.array_equal(back, got), why
        print(f"{name} {opts}: bit-equal with the engine's inverse_dynamics on the perturbed states: {bit_equal}")
        eng.close()
    print(f"{name}: max |sweep - oracle| / max|tau| = {worst_o:.2e}, max |sweep - engine| / max|tau| = {worst_e:.2e}")


def test_jacobians_are_the_forward_differences_of_the_sweep():
    from flobaroid_amd import excitation as exc

    name = "kuka_lwr4-fr"
    t = _topo(name)
    n, C, T = t.num_dofs, 3, 7
    eng = _engine(name, t)
    st, vs, x_std, rng = _batch(name, t, C, T, 3)
    sample = rng.integers(0, T, (C, n)).astype(np.int64)
    sw = eng.torque_row_sweep(st, C, sample, x_std, EPS)
    jac = exc.candidate_torque_jacobians(eng, st, C, sample, x_std, EPS)
    assert np.array_equal(jac["tau"], sw[..., 0])
    for i, k in enumerate(("dtau_dq", "dtau_ddq_state", "dtau_dddq")):
        assert jac[k].shape == (C, n, n) and np.array_equal(jac[k], (sw[..., 1 + i * n:1 + (i + 1) * n] - sw[..., :1]) / EPS), k
    # the mass matrix is symmetric and positive: d tau_n / d ddq_n > 0 (a wrong kind or joint offset would not survive this)
    assert np.all(np.diagonal(jac["dtau_dddq"], axis1=1, axis2=2) > 0)
    eng.close()


def test_indices_out_of_range_and_bad_arguments_are_refused_and_the_handle_survives():
    from flobaroid_amd._lib import FbrError

    name = "kuka_lwr4-stribeck"
    t = _topo(name)
    n, C, T = t.num_dofs, 2, 5
    eng = _engine(name, t)
    st, vs, x_std, rng = _batch(name, t, C, T, 9)
    ok_s, ok_j = np.zeros((C, 3), dtype=np.int64), np.zeros((C, 3), dtype=np.int32)
    for opts_fused in (1, 0):
        eng.set_option("fused_id", opts_fused)
        for bad_s, bad_j in ((T, 0), (-1, 0), (0, n), (0, -1)):
            s, j = ok_s.copy(), ok_j.copy()
            s[1, 2], j[1, 2] = bad_s, bad_j
            with pytest.raises(FbrError, match="code -1"):
                eng.torque_row_sweep(st, C, s, x_std, EPS, joint=j, vel_sign=vs)
    eng.set_option("fused_id", 1)
    for eps in (0.0, float("nan"), float("inf")):
        with pytest.raises(FbrError, match="code -1"):
            eng.torque_row_sweep(st, C, ok_s, x_std, eps, joint=ok_j, vel_sign=vs)
    with pytest.raises(FbrError, match="code -1"):  # joint NULL needs nrows == n
        eng.torque_row_sweep(st, C, ok_s, x_std, EPS, vel_sign=vs)
    with pytest.raises(FbrError, match="code -1"):  # nrows < 1
        eng.torque_row_sweep(st, C, np.zeros((C, 0), dtype=np.int64), x_std, EPS, joint=np.zeros((C, 0), dtype=np.int32), vel_sign=vs)
    with pytest.raises(FbrError, match="code -1"):  # not a multiple of ncand
        eng.torque_row_sweep({k: v[:9] for k, v in st.items()}, C, ok_s, x_std, EPS, joint=ok_j, vel_sign=vs[:9])
    with pytest.raises(FbrError, match="code -1"):  # Stribeck without vel_sign
        eng.torque_row_sweep(st, C, ok_s, x_std, EPS, joint=ok_j)
    with pytest.raises(FbrError, match="code -1"):
        eng.torque_row_sweep(st, C, ok_s, x_std[:5], EPS, joint=ok_j, vel_sign=vs)
    got = eng.torque_row_sweep(st, C, ok_s, x_std, EPS, joint=ok_j, vel_sign=vs)
    tau = eng.inverse_dynamics(st, x_std, vel_sign=vs)
    assert np.abs(got[:, :, 0] - tau[[0, T], 0][:, None]).max() <= 1e-13 * np.abs(tau).max()
    eng.close()


@pytest.mark.parametrize("depth", [4, 5, 8, 9, 12, 13, 24, 25])
def test_joint_paths_at_the_instance_thresholds(depth):
    """A chain of `depth` joints: the register-stack instance of that depth (4, 8, 12, FBR_KINID_MAXD = 24), 25 the two-kernel route; every
    entry against the engine's own inverse_dynamics on the perturbed states"""
    from flobaroid_amd._lib import Engine

    rng = np.random.default_rng([31, depth])
    t = random_topology(rng, depth + 1, p_fixed=0.0, branchiness=0.0, p_prismatic=0.2)
    assert t.num_dofs == depth
    floating = bool(depth % 2)
    C, T, n = 2, 3, depth
    st = random_states(t, C * T, rng, floating)
    sample = rng.integers(0, T, (C, n)).astype(np.int64)
    eng = Engine(t, floating=floating)
    got = eng.torque_row_sweep(st, C, sample, t.x_std(), EPS)
    pert, _, jn = _perturbed(st, None, T, sample, None, n)
    tau = eng.inverse_dynamics(pert, t.x_std())
    want = tau[np.arange(jn.size), (6 if floating else 0) + jn].reshape(got.shape)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(tau).max(), depth
    eng.close()
