"""fbr_dopt_terms on the device (Engine.dopt_terms): eigenvalues, D-optimality terms and weight matrices of candidate Grams against the
50-digit reference and its bars (tests/dopt_reference.py), at n = 213 against residuals and eigvalsh; exact power-of-two scaling, isolation
of a NaN candidate, chunking, memory spaces, refusals; and the ``device_spectrum=True`` routes of flobaroid_amd.excitation end to end.

Figures of a run are printed (worst error / bar); they are recorded in DESIGN.md."""
import numpy as np
import pytest

import dopt_reference as dr
import fourier_gradient_restatement as fgr
from common import load_topo

pytestmark = pytest.mark.gpu
EPS = dr.EPS


@pytest.fixture(scope="module")
def eng():
    from flobaroid_amd._lib import Engine

    e = Engine(load_topo("threeLinks"))
    yield e
    e.close()


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in d.items()}


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("name", dr.CASES)
def test_families_within_the_bars_in_both_memory_spaces(eng, name):
    G, cols, reg, prior, scale = dr.case(name)
    out = eng.dopt_terms(_dev(G), cols, reg, prior=prior, scale=scale, eigenvalues=True, weights=True)
    assert all(hasattr(v, "cpu") for v in out.values()) and out["n_observable"].dtype.is_floating_point is False
    got = _np(out)
    w = dr.check_against_reference(name, got, "device")
    print(name, "n =", len(cols), "worst error / bar:", {k: float(f"{v:.3g}") for k, v in w.items()})
    # two calls, the host-resident G, and a call without eig / Cmat: the same bits
    assert _same(got, _np(eng.dopt_terms(_dev(G), cols, reg, prior=prior, scale=scale, eigenvalues=True, weights=True)))
    host = eng.dopt_terms(G, cols, reg, prior=prior, scale=scale, eigenvalues=True, weights=True)
    assert all(isinstance(v, np.ndarray) for v in host.values()) and _same(got, host)
    bare = _np(eng.dopt_terms(_dev(G), cols, reg, prior=prior, scale=scale))
    assert set(bare) == {"neg_log_det", "lambda_max", "delta", "n_observable", "status"} and all(np.array_equal(bare[k], got[k]) for k in bare)
    assert _same(bare, eng.dopt_terms(G, cols, reg, prior=prior, scale=scale))


def test_zero_matrix(eng):
    G, cols, reg, _, _ = dr.case("zero")
    got = _np(eng.dopt_terms(_dev(G), cols, reg, eigenvalues=True, weights=True))
    assert np.all(got["eig"] == 0.0) and np.all(got["lambda_max"] == 0.0) and np.all(got["delta"] == reg * 1e-30)
    assert np.all(got["n_observable"] == 0) and np.all(np.isfinite(got["Cmat"])) and np.all(got["status"] == 0)
    want = -2.0 / (reg * 1e-30)  # (M + delta I = delta I)
    assert np.all(got["Cmat"][0][~np.eye(4, dtype=bool)] == 0.0) and np.abs(np.diag(got["Cmat"][0]) / want - 1.0).max() <= 4 * EPS


def test_reg_zero_on_a_singular_matrix_raises_for_that_candidate_only(eng):
    Ms = [np.eye(5), 2.0 * np.eye(5) + 0.5, np.diag([1.0, 1.0, 0.0, 1.0, 1.0]), np.diag([3.0, 1.0, 2.0, 1.0, 5.0])]
    G, cols = dr.embed(Ms, None, np.random.default_rng(4))
    with pytest.raises(np.linalg.LinAlgError, match=r"candidates \[2\]") as ei:
        eng.dopt_terms(_dev(G), cols, 0.0, weights=True)
    assert ei.value.status.tolist() == [0, 0, 2, 0]
    got = _np(eng.dopt_terms(_dev(G), cols, 0.0, eigenvalues=True))  # without the weights the terms stand
    assert got["status"].tolist() == [0, 0, 0, 0] and np.all(got["delta"] == 0.0) and got["n_observable"].tolist() == [5, 5, 4, 5]
    assert np.abs(got["eig"][2] - [0, 1, 1, 1, 1]).max() <= dr.bar_lambda(5)


@pytest.mark.parametrize("case", dr.ROBOTS, ids=lambda c: f"{c[0]}-{c[3]}x{c[4]}")
def test_oracle_grams_of_the_robots(eng, case):
    """threeLinks (nb = 24) and KUKA with friction (nb = 64) against the 50-digit reference, WALK-MAN (nb = 213) with 70 and with 5 samples
    (175 rows for 213 columns) by residuals and against eigvalsh: tests/dopt_reference.py check_robot"""
    G, cols = dr.oracle_grams(*case)
    scale = np.linspace(0.5, 1.5, case[3])
    assert G.shape[1] > len(cols) + 1
    dr.check_robot(case, _np(eng.dopt_terms(_dev(G), cols, 1e-4, scale=scale, eigenvalues=True, weights=True)), scale, where="device")


def test_power_of_two_scaling_is_exact(eng):
    G, cols, reg, _, _ = dr.case("logspace24")
    G = G * 2.0 ** 210  # (so that lambda_max of 2^-300 G stays above the floor 1e-30 under delta)
    base = _np(eng.dopt_terms(_dev(G), cols, reg, eigenvalues=True, weights=True))
    for p in (300, -300):
        got = _np(eng.dopt_terms(_dev(G * 2.0 ** p), cols, reg, eigenvalues=True, weights=True))
        for k in ("eig", "lambda_max", "delta"):
            assert np.array_equal(got[k], base[k] * 2.0 ** p), (p, k)
        assert np.array_equal(got["Cmat"], base["Cmat"] * 2.0 ** -p) and np.array_equal(got["n_observable"], base["n_observable"])


def test_a_nan_stays_in_its_candidate(eng):
    G, cols, reg, _, _ = dr.case("logspace24")
    G = np.concatenate([G, G[:2] * 3.0])
    clean = _np(eng.dopt_terms(_dev(G), cols, reg, eigenvalues=True, weights=True))
    G[2, cols[5], cols[2]] = np.nan
    with pytest.raises(np.linalg.LinAlgError, match=r"candidates \[2\]"):
        eng.dopt_terms(_dev(G), cols, reg, weights=True)
    got = _np(eng.dopt_terms(_dev(G), cols, reg, eigenvalues=True))
    for c in (0, 1, 3, 4):
        assert all(np.array_equal(got[k][c], clean[k][c]) for k in got), c
    assert got["status"].tolist() == [0, 0, 1, 0, 0] and got["n_observable"][2] == 0 and np.all(np.isnan(got["eig"][2]))
    assert all(np.isnan(got[k][2]) for k in ("neg_log_det", "lambda_max", "delta"))


def test_more_candidates_than_one_grid_chunk(eng):
    C = 70000
    rng = np.random.default_rng(8)
    a, b, c = 1.0 + rng.random(C), rng.uniform(-0.9, 0.9, C), 1.5 + rng.random(C)  # (positive definite: a c - b^2 > 0.69)
    G = rng.standard_normal((C, 3, 3))
    G[:, 2, 2], G[:, 0, 0], G[:, 0, 2] = a, c, b  # cols = (2, 0): M = [[a, .], [b, c]], b = G[cols[1], cols[0]]
    got = _np(eng.dopt_terms(_dev(G), [2, 0], 1e-3, eigenvalues=True))
    al, bl, cl = (x.astype(np.longdouble) for x in (a, b, c))
    h = np.sqrt(((al - cl) / 2) ** 2 + bl * bl)
    want = np.stack([((al + cl) / 2 - h), ((al + cl) / 2 + h)], axis=1)
    err = np.abs(got["eig"] - want.astype(np.float64)).max(axis=1) / want[:, 1].astype(np.float64)
    print("70000 candidates of n = 2: worst eigenvalue error", err.max(), "bar", dr.bar_lambda(2))
    assert err.max() <= dr.bar_lambda(2) and np.all(got["status"] == 0) and np.array_equal(got["lambda_max"], got["eig"][:, 1])
    dl = 1e-3 * want[:, 1:]
    nld = -np.sum(np.log(want + dl), axis=1).astype(np.float64)
    assert np.abs(got["neg_log_det"] - nld).max() <= dr.bar_neg_log_det(2, 1e-3)
    assert np.array_equal(got["n_observable"], np.sum(want > dl, axis=1))


def test_refusals(eng):
    from flobaroid_amd._lib import FBR_MAX_DOPT_COLUMNS, FbrError

    G = np.zeros((2, 6, 6))
    big = np.zeros((1, FBR_MAX_DOPT_COLUMNS + 2, FBR_MAX_DOPT_COLUMNS + 2))
    with pytest.raises(FbrError, match="FBR_MAX_DOPT_COLUMNS = 512"):
        eng.dopt_terms(big, np.arange(FBR_MAX_DOPT_COLUMNS + 1))
    with pytest.raises(FbrError, match="out of range or twice"):
        eng.dopt_terms(G, [1, 3, 1])
    with pytest.raises(FbrError, match="out of range or twice"):
        eng.dopt_terms(G, [1, 6])
    with pytest.raises(FbrError, match="out of range or twice"):
        eng.dopt_terms(G, [-1, 2])
    with pytest.raises(FbrError, match="ngroups < 1"):
        eng.dopt_terms(np.zeros((0, 6, 6)), [1, 2])
    with pytest.raises(FbrError, match="reg is negative or not finite"):
        eng.dopt_terms(G, [1, 2], reg=-1e-4)
    with pytest.raises(FbrError, match="reg is negative or not finite"):
        eng.dopt_terms(G, [1, 2], reg=float("nan"))
    with pytest.raises(FbrError, match="ncols outside"):
        eng.dopt_terms(G, np.arange(7))
    top = eng.dopt_terms(big[:, :FBR_MAX_DOPT_COLUMNS, :FBR_MAX_DOPT_COLUMNS] + np.eye(FBR_MAX_DOPT_COLUMNS), np.arange(FBR_MAX_DOPT_COLUMNS))
    assert abs(top["lambda_max"][0] - 1.0) <= dr.bar_lambda(FBR_MAX_DOPT_COLUMNS) and top["n_observable"][0] == FBR_MAX_DOPT_COLUMNS  # (the limit itself is served)


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end: the device_spectrum routes of flobaroid_amd.excitation
# ---------------------------------------------------------------------------------------------------------------------------------
def _forbid_host_route(monkeypatch):
    from flobaroid_amd import estimation as est
    from flobaroid_amd import excitation as exc

    def no(*a, **k):
        raise AssertionError("the host route was taken under device_spectrum=True")

    monkeypatch.setattr(est, "d_optimality_batch_terms", no)
    monkeypatch.setattr(exc, "dopt_weight_matrices", no)


def test_objectives_with_the_spectrum_on_the_device(monkeypatch, tmp_path):
    from flobaroid_amd import excitation as exc
    from test_gpu_dopt_gradient import _engine, _independent_columns, _random_candidates

    topo, eng = _engine("kuka_lwr4", 0, 0)
    C, T, freq = 3, 96, 50.0
    cands = _random_candidates(topo, eng.n, C, 2, False, np.random.default_rng(23))
    ic = _independent_columns(eng, topo)
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    args = (eng, cands, T, freq, topo.x_std(), ic, limits, topo.dof_names, {"doptRegularization": 1e-4})
    base = exc.candidate_objectives_from_coefficients(*args, dopt_scale=0.5)
    off = exc.candidate_objectives_from_coefficients(*args, dopt_scale=0.5, device_spectrum=False)
    for k in base:
        if k != "ag_cache":
            assert np.array_equal(np.asarray(base[k]), np.asarray(off[k]), equal_nan=True), k
    assert all(np.array_equal(base["ag_cache"][k], off["ag_cache"][k]) for k in base["ag_cache"])
    d0 = exc.candidate_dopt_from_coefficients(eng, cands, T, freq, ic)
    with pytest.raises(ValueError, match="host route"):
        exc.candidate_objectives_from_coefficients(*args[:-1], {"useBasisProjection": True}, device_spectrum=True)
    with pytest.raises(ValueError, match="host route"):
        exc.candidate_gradients_from_coefficients(*args[:-1], {"useBasisProjection": 1}, device_spectrum=True)
    _forbid_host_route(monkeypatch)
    dev = exc.candidate_objectives_from_coefficients(*args, dopt_scale=0.5, device_spectrum=True)
    n = len(ic)
    bar = dr.bar_neg_log_det(n, 1e-4) * 0.5
    print("objectives: max |f - f_host|", np.abs(dev["f"] - base["f"]).max(), "bar", bar)
    assert np.array_equal(dev["g"], base["g"]) and all(np.array_equal(base["ag_cache"][k], dev["ag_cache"][k]) for k in base["ag_cache"])
    assert np.array_equal(dev["n_observable"], base["n_observable"])
    assert np.abs(dev["f"] - base["f"]).max() <= bar and np.abs(dev["dopt"] - base["dopt"]).max() <= bar
    # a configuration that says useBasisProjection: 0 -- what Model.__init__ writes into the caller's option dict -- takes the device route
    # and changes no bit; so does the very dict a Model was built from
    from flobaroid_amd.model import Model

    path = str(tmp_path / "kuka_lwr4.topology.json")
    topo.save_json(path)
    opt = dict(floatingBase=0, identifyFrictionSimultaneously=0, identifySymmetricVelFriction=1, identifyGravityParamsOnly=0, simulateTorques=0,
               useAPriori=0, useStructuralRegressor=1, skipSamples=0, startOffset=0, verbose=0, showTiming=0, filterRegressor=0,
               estimateWith="std", randomSamples=500, minTol=1e-4, selectBlocksFromMeasurements=0, doptRegularization=1e-4)
    Model(opt, path)
    assert opt["useBasisProjection"] == 0
    for config in ({"doptRegularization": 1e-4, "useBasisProjection": 0}, opt):
        again = exc.candidate_objectives_from_coefficients(*args[:-1], config, dopt_scale=0.5, device_spectrum=True)
        assert np.array_equal(again["f"], dev["f"]) and np.array_equal(again["g"], dev["g"]) and np.array_equal(again["n_observable"], dev["n_observable"])
    d1 = exc.candidate_dopt_from_coefficients(eng, cands, T, freq, ic, device_spectrum=True)
    assert np.abs(d1 - d0).max() <= dr.bar_neg_log_det(n, 1e-4)
    # the whole gradient entry point takes the same route: f, g as above; the D-optimality gradient moves by what the difference of the two
    # C (1e-13 of max|C|) leaves behind the forward difference over eps = 1e-7, far inside that sweep's own bar of 1e-10 / eps = 1e-3
    monkeypatch.undo()
    h = exc.candidate_gradients_from_coefficients(*args[:-1], opt, dopt_scale=0.5)
    _forbid_host_route(monkeypatch)
    calls = []
    real = eng.dopt_terms
    monkeypatch.setattr(eng, "dopt_terms", lambda *a, **k: (calls.append(k.get("weights", False)), real(*a, **k))[1])
    d = exc.candidate_gradients_from_coefficients(*args[:-1], opt, dopt_scale=0.5, device_spectrum=True)
    assert calls == [True]  # one call serves the terms and the weight matrices
    assert np.array_equal(d["g"], h["g"]) and np.abs(d["f"] - h["f"]).max() <= bar
    for k in h["obj_grad"]:
        assert np.array_equal(d["soft_grad"][k], h["soft_grad"][k]) and all(np.array_equal(d["con_grad"][k], h["con_grad"][k]) for k in h["con_grad"])
        scale_k = np.abs(h["dopt_grad"][k]).max()
        assert scale_k > 0 or k == "q_range"
        assert np.abs(d["dopt_grad"][k] - h["dopt_grad"][k]).max() <= 1e-5 * max(scale_k, 1e-300), k
    eng.close()


@pytest.mark.parametrize("name,floating,C,T,k,bounded", [("kuka_lwr4", 0, 3, 96, 1, False), ("walkman_apriori", 1, 2, 70, 3, True)],
                         ids=["kuka-3x96", "walkman-fb-2x70-sub3"])
def test_gradient_with_the_spectrum_on_the_device(monkeypatch, name, floating, C, T, k, bounded):
    """candidate_dopt_gradient_from_coefficients(device_spectrum=True) against the CPU assembly of test_gpu_dopt_gradient.py (oracle
    regressors, forward differences, that file's per-sensitivity bar 1e-10 max|score| / eps), with C from Engine.dopt_terms on the host."""
    from flobaroid_amd import excitation as exc
    from oracle.oracle import OracleModel
    from test_gpu_dopt_gradient import _engine, _independent_columns, _random_candidates

    topo, eng = _engine(name, floating, 0)
    n, rows, P = eng.n, eng.rows, eng.cols
    freq, eps, nh = 50.0, 1e-7, 2
    cands = _random_candidates(topo, n, C, nh, bounded, np.random.default_rng(23))
    ic = _independent_columns(eng, topo)
    kw = dict(dopt_scale=0.5, epsilon=eps, subsample=k)
    f0, g0 = exc.candidate_dopt_gradient_from_coefficients(eng, cands, T, freq, ic, **kw)
    f00, g00 = exc.candidate_dopt_gradient_from_coefficients(eng, cands, T, freq, ic, device_spectrum=False, **kw)
    assert np.array_equal(f0, f00) and all(np.array_equal(g0[key], g00[key]) for key in g0)
    _forbid_host_route(monkeypatch)
    f, grad = exc.candidate_dopt_gradient_from_coefficients(eng, cands, T, freq, ic, device_spectrum=True, **kw)
    assert np.abs(f - f0).max() <= dr.bar_neg_log_det(len(ic), 1e-4) * 0.5
    st = exc.candidate_states(eng, cands, T, freq, device=False)
    Cm = eng.dopt_terms(eng.gram_grouped(st, C), ic, 1e-4, scale=0.5, weights=True)["Cmat"]
    cols = np.asarray(ic)
    om = OracleModel(topo, floating=bool(floating), fric=False)
    Ts = (T + k - 1) // k
    sub = {key: v.reshape(C, T, -1)[:, ::k].reshape(C * Ts, -1) for key, v in st.items()}
    S = C * Ts
    Y0 = om.regressor(sub).reshape(C, Ts * rows, P)
    W = np.zeros_like(Y0)
    W[:, :, cols] = np.einsum("grk,gkj->grj", Y0[:, :, cols], Cm)
    W = W.reshape(S, rows * P)
    base = np.einsum("sx,sx->s", W, Y0.reshape(S, rows * P))
    sens = np.zeros((3, S, n))
    smax = np.abs(base).max()
    for kind, key in enumerate(("q", "dq", "ddq")):
        for d in range(n):
            pert = {kk: v.copy() for kk, v in sub.items()}
            pert[key][:, d] += eps
            sc = np.einsum("sx,sx->s", W, om.regressor(pert).reshape(S, rows * P))
            smax = max(smax, np.abs(sc).max())
            sens[kind, :, d] = (sc - base) * (k / eps)
    A, B = np.stack([c["a"] for c in cands]), np.stack([c["b"] for c in cands])
    t = (np.arange(Ts) * k).astype(np.longdouble) / np.longdouble(freq)
    s_bar = 1e-10 * smax / eps * k
    worst = 0.0
    for c in range(C):
        qr = cands[c]["q_range"]
        s = [x.reshape(C, Ts, n)[c] for x in sens]
        want, _ = fgr.chain(cands[c]["wf"], qr, A[c], B[c], s[0], s[1], s[2], t)
        one = np.ones((Ts, n))
        _, dsum = fgr.chain(cands[c]["wf"], qr, A[c], B[c], one, one, one, t)
        got = np.concatenate([[grad["wf"][c]], grad["q_offset"][c], grad["q_range"][c], grad["a"][c].ravel(), grad["b"][c].ravel()])
        err = np.abs(got - want.astype(np.float64))
        bar = s_bar * dsum.astype(np.float64)
        live = np.ones(got.size, dtype=bool) if bounded else np.r_[np.ones(1 + n, bool), np.zeros(n, bool), np.ones(2 * n * nh, bool)]
        worst = max(worst, float((err[live] / bar[live]).max()))
        assert np.all(err[live] <= bar[live]), (c, int(np.argmax(err / np.maximum(bar, 1e-300))), float(err.max()))
        assert np.linalg.norm(want) > 0
    print("device_spectrum gradient", name, "worst err / bar:", worst)
    eng.close()
