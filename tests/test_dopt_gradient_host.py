"""Host pieces of the D-optimality gradient of candidate trajectories (excitation.candidate_dopt_gradient_from_coefficients): the series
Jacobian restated in tests/fourier_gradient_restatement.py against SymPy's own derivative, the weight matrices against the brute-force
expression on oracle regressors, and the map onto the reference's variable vector."""
import numpy as np
import pytest

import fourier_gradient_restatement as fgr
from common import load_topo, random_states


def _sympy_jacobian(bounded, nh):
    """lambdified d(q, dq, ddq)/dp from sympy.diff of the series expression itself; p = [wf, q_offset, q_range, a.., b..]"""
    import sympy as sp

    t, wf, qo, qr = sp.symbols("t wf qo qr", real=True)
    a = sp.symbols(f"a1:{nh + 1}", real=True)
    b = sp.symbols(f"b1:{nh + 1}", real=True)
    if bounded:
        q = qo + qr * sp.tanh(sum(b[l - 1] * sp.cos(wf * l * t) + a[l - 1] * sp.sin(wf * l * t) for l in range(1, nh + 1)))
        dq = sp.diff(q, t)
    else:
        dq = sum(a[l - 1] * sp.cos(wf * l * t) + b[l - 1] * sp.sin(wf * l * t) for l in range(1, nh + 1))
        q = qo + sum(a[l - 1] / (wf * l) * sp.sin(wf * l * t) - b[l - 1] / (wf * l) * sp.cos(wf * l * t) for l in range(1, nh + 1))
    ddq = sp.diff(dq, t)
    params = [wf, qo, qr, *a, *b]
    exprs = [[sp.diff(e, p) for p in params] for e in (q, dq, ddq)]
    return sp.lambdify([t, wf, qo, qr, *a, *b], exprs, "mpmath")


@pytest.mark.parametrize("bounded", [False, True])
def test_series_jacobian_matches_sympy(bounded):
    """Agreement to rounding, entry by entry: 1e-12 * max(1, largest phase wf l t) * |value| (the phase rounding eps * x is what sin and cos
    see); an entry that is identically zero must be exactly zero.  SymPy's derivative is evaluated in 40-digit mpmath."""
    import mpmath as mp

    mp.mp.dps = 40
    nh = 3
    f = _sympy_jacobian(bounded, nh)
    rng = np.random.default_rng(5)
    wf, qo, qr = 2 * np.pi * 0.1, 0.3, 0.8
    a, b = rng.uniform(-0.6, 0.6, nh), rng.uniform(-0.6, 0.6, nh)
    t = np.array([0.0, 0.01, 0.37, 2.5, 19.99, 63.0])
    J = fgr.series_jacobian(wf, qr if bounded else None, a, b, t)
    for i, ti in enumerate(t):
        want = np.array([[float(v) for v in row] for row in f(ti, wf, qo, qr, *a, *b)])
        phase = max(1.0, wf * nh * ti)
        for k in range(3):
            bar = 1e-12 * phase * np.abs(want[k])
            assert np.all(np.abs(J[k, i] - want[k]) <= bar), (bounded, ti, k, np.abs(J[k, i] - want[k]).max())
    # and the series itself is the one differentiated
    q, dq, ddq = fgr.series(wf, qo, qr if bounded else None, a, b, t)
    h = 1e-6
    qp, _, _ = fgr.series(wf, qo, qr if bounded else None, a, b, t + h)
    qm, _, _ = fgr.series(wf, qo, qr if bounded else None, a, b, t - h)
    assert np.abs((qp - qm) / (2 * h) - dq).max() <= 1e-7 * max(1.0, np.abs(dq).max())


def _oracle_regressor(name, floating, S, seed):
    from oracle.oracle import OracleModel

    topo = load_topo(name)
    st = random_states(topo, S, np.random.default_rng(seed), floating, use_limits=True)
    return topo, OracleModel(topo, floating=floating).regressor(st)


@pytest.mark.parametrize("name,floating", [("threeLinks", True), ("kuka_lwr4", False)])
@pytest.mark.parametrize("variant", ["plain", "prior", "basis"])
def test_weight_matrices_match_brute_force(name, floating, variant):
    """W = Y[:, cols] C against -2 scale YBase (YBase^T YBase [+ prior] + delta I)^-1 Pb^T formed row by row from oracle regressors.
    Bar 1e-9 of the largest weight: the regularised matrix has condition <= 1 / reg + 1 = 1e4, so both inverses carry about 1e4 eps
    times a modest dimension factor (~1e2) of relative error."""
    import scipy.linalg as sla

    from flobaroid_amd import excitation as exc

    topo, Y = _oracle_regressor(name, floating, 40, 3)
    rng = np.random.default_rng(11)
    P = Y.shape[1]
    G = Y.T @ Y
    rank = np.linalg.matrix_rank(Y)
    ic = np.sort(sla.qr(Y, pivoting=True, mode="r")[1][:rank])
    reg, scale = 1e-4, 0.37
    prior = None
    if variant == "prior":
        Z = rng.standard_normal((rank + 3, rank))
        prior = Z.T @ Z * (np.trace(G) / P)
    if variant == "basis":
        B = np.linalg.svd(Y, full_matrices=False)[2][:rank].T  # (P, rank): an orthonormal basis of the row space
        YB, Pb_T = Y @ B, B.T
        Cm, cols = exc.dopt_weight_matrices(G[None], ic, reg, scale, B=B)
        assert list(cols) == list(range(P))
    else:
        YB = Y[:, ic]
        Pb_T = np.zeros((rank, P))
        Pb_T[np.arange(rank), ic] = 1.0
        Cm, cols = exc.dopt_weight_matrices(G[None], ic, reg, scale, YtY_prior=prior)
        assert list(cols) == list(ic)
    M = YB.T @ YB + (0 if prior is None else prior)
    delta = reg * np.linalg.eigvalsh(M)[-1]
    want = -2.0 * scale * np.linalg.solve(M + delta * np.eye(rank), YB.T).T @ Pb_T
    got = np.zeros_like(want)
    got[:, cols] = Y[:, cols] @ Cm[0]
    assert Cm.shape == (1, len(cols), len(cols))
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_weight_matrices_take_delta_per_candidate():
    from flobaroid_amd import excitation as exc

    _, Y = _oracle_regressor("threeLinks", False, 30, 4)
    G = np.stack([Y[:45].T @ Y[:45], 9.0 * (Y[45:].T @ Y[45:])])
    ic = np.arange(0, Y.shape[1], 3)
    Cm, _ = exc.dopt_weight_matrices(G, ic, 1e-3, [1.0, 2.0])
    for c in range(2):
        one, _ = exc.dopt_weight_matrices(G[c], ic, 1e-3, [1.0, 2.0][c])
        assert np.array_equal(one[0], Cm[c])


def test_gradient_maps_onto_the_optimizer_variables():
    """[wf | q0 (n) | a ragged | b ragged]: classic q0 through nf_d * deg_factor, bounded through q_center only; ``exact`` adds the q_range
    and clip terms."""
    from flobaroid_amd import excitation as exc

    nf = [2, 1, 3]
    n, nh = 3, 3
    rng = np.random.default_rng(0)
    g = {"wf": np.float64(0.7), "q_offset": rng.standard_normal(n), "q_range": rng.standard_normal(n), "a": rng.standard_normal((n, nh)),
         "b": rng.standard_normal((n, nh))}
    cand = {"q_range": None}
    v = exc.gradient_to_optimizer_variables(g, cand, nf, use_deg=True, bounded=False)
    assert v.shape == (1 + n + 2 * sum(nf),)
    assert v[0] == 0.7
    assert np.allclose(v[1:4], g["q_offset"] * np.array(nf) * np.pi / 180.0, rtol=1e-15, atol=0)
    assert np.array_equal(v[4:10], np.concatenate([g["a"][0, :2], g["a"][1, :1], g["a"][2, :3]]))
    assert np.array_equal(v[10:16], np.concatenate([g["b"][0, :2], g["b"][1, :1], g["b"][2, :3]]))
    vb = exc.gradient_to_optimizer_variables(g, {"q_range": np.ones(n)}, nf, use_deg=False, bounded=True)
    assert np.array_equal(vb[1:4], g["q_offset"]) and np.array_equal(vb[4:], v[4:])
    # exact: joint 0 inside and nearer the lower limit (+0.95), joint 1 nearer the upper (-0.95), joint 2 clipped (0)
    lim = [(-1.0, 1.0)] * 3
    q0 = np.array([-0.2, 0.4, 1.5])
    ve = exc.gradient_to_optimizer_variables(g, {"q_range": np.ones(n)}, nf, use_deg=False, bounded=True, exact=True, joint_limits=lim, q0=q0)
    want = np.array([g["q_offset"][0] + 0.95 * g["q_range"][0], g["q_offset"][1] - 0.95 * g["q_range"][1], 0.0])
    assert np.allclose(ve[1:4], want, rtol=1e-15, atol=0)
    # and it is the derivative of fourier_coefficients' own q_offset / q_range
    h = 1e-6
    for j in range(2):
        e = np.zeros(n)
        e[j] = h
        cp = exc.fourier_coefficients([[0]] * n, [[0]] * n, q0 + e, [1] * n, joint_limits=lim)
        cm = exc.fourier_coefficients([[0]] * n, [[0]] * n, q0 - e, [1] * n, joint_limits=lim)
        fd = (g["q_offset"] @ (cp["q_offset"] - cm["q_offset"]) + g["q_range"] @ (cp["q_range"] - cm["q_range"])) / (2 * h)
        assert abs(fd - ve[1 + j]) <= 1e-8 * max(1.0, abs(fd))


# ------------------------------------------------------------------------------------------------------------------------------------
# Chain mathematics: the assembled gradient against differences of the objective itself
# ------------------------------------------------------------------------------------------------------------------------------------
# largest |assembled - Richardson| / |gradient|_2 over the checked coordinates and candidates of the committed seeds, measured with
# OpenBLAS on x86-64 (printed by the test); the bar is 10 x that (other BLAS builds), capped at 1e-4
CHAIN_MEASURED = {"kuka_lwr4": 2.2e-8, "threeLinks": 9.9e-9}


def _chain_fixture(name, floating, bounded, C, T, nf, seed):
    from oracle.oracle import OracleModel

    import scipy.linalg as sla

    topo = load_topo(name)
    om = OracleModel(topo, floating=floating)
    n = topo.num_dofs
    rng = np.random.default_rng(seed)
    Yr = om.regressor(random_states(topo, 300, rng, floating, use_limits=True))
    R, piv = sla.qr(Yr, pivoting=True, mode="r")
    d = np.abs(np.diag(R))
    ic = np.sort(piv[: int(np.sum(d > 1e-9 * d[0]))])
    nh = max(nf)
    cands = []
    for _ in range(C):
        A, B = rng.uniform(-0.3, 0.3, (n, nh)), rng.uniform(-0.3, 0.3, (n, nh))
        for j in range(n):
            A[j, nf[j]:] = 0.0
            B[j, nf[j]:] = 0.0
        cands.append({"wf": 2 * np.pi * rng.uniform(0.08, 0.12), "a": A, "b": B, "q_offset": rng.uniform(-0.2, 0.2, n),
                      "q_range": rng.uniform(0.4, 0.9, n) if bounded else None})
    return topo, om, ic, cands


def _states_of(cand, n, t, floating):
    cols = [fgr.series(cand["wf"], cand["q_offset"][j], None if cand["q_range"] is None else cand["q_range"][j], cand["a"][j], cand["b"][j], t)
            for j in range(n)]
    st = {"q": np.stack([c[0] for c in cols], 1), "dq": np.stack([c[1] for c in cols], 1), "ddq": np.stack([c[2] for c in cols], 1)}
    if floating:
        st.update(base_vel=np.zeros((t.size, 6)), base_acc=np.zeros((t.size, 6)), rpy=np.zeros((t.size, 3)))
    return st


def cpu_gradient_assembly(om, cand, n, t, floating, ic, reg, scale, eps, subsample=1):
    """The pipeline of candidate_dopt_gradient_from_coefficients on the CPU: oracle regressors, dopt_weight_matrices, forward differences of
    sum(W * Y) with the same eps, the restatement's chain.  Returns (gradient in fbr_fourier_gradient's layout, delta_0)."""
    from flobaroid_amd import excitation as exc

    st = _states_of(cand, n, t, floating)
    Y = om.regressor(st)
    G = Y.T @ Y
    Cm, cols = exc.dopt_weight_matrices(G, ic, reg, scale)
    delta0 = reg * np.linalg.eigvalsh(G[np.ix_(ic, ic)])[-1]
    k = int(subsample)
    sub = {key: v[::k] for key, v in st.items()}
    S = sub["q"].shape[0]
    Ys = om.regressor(sub)
    W = np.zeros_like(Ys)
    W[:, cols] = Ys[:, cols] @ Cm[0]
    W = W.reshape(S, -1)
    base = np.einsum("sx,sx->s", W, Ys.reshape(S, -1))
    sens = np.zeros((3, S, n))
    for kind, key in enumerate(("q", "dq", "ddq")):
        for d in range(n):
            pert = {kk: v.copy() for kk, v in sub.items()}
            pert[key][:, d] += eps
            sens[kind, :, d] = (np.einsum("sx,sx->s", W, om.regressor(pert).reshape(S, -1)) - base) * (k / eps)
    g, _ = fgr.chain(cand["wf"], cand["q_range"], cand["a"], cand["b"], sens[0], sens[1], sens[2], t[::k])
    return g.astype(np.float64), delta0


@pytest.mark.parametrize("name,floating,bounded,C,T,nf", [("kuka_lwr4", False, False, 3, 96, [2] * 7), ("threeLinks", True, True, 2, 64, [2, 1, 2])],
                         ids=["kuka-3x96", "threeLinks-fb-bounded"])
def test_assembled_gradient_is_the_derivative_of_the_frozen_delta_objective(name, floating, bounded, C, T, nf):
    """The gradient assembled from oracle regressors (forward difference eps = 1e-7 of sum(W * Y), W = Y[:, cols] C, chained with the
    restatement's Jacobian) against Richardson-extrapolated central differences (steps h and h / 2, h = 1e-3) of the objective itself,
    F(theta) = -scale logdet(M(theta) + delta_0 I) with delta_0 frozen at theta_0 -- independent of the weight formula, its sign and factor,
    and of the layout of the chain.  Coordinates: wf, one q_offset, two a, two b per candidate.

    Observed on the committed seeds, largest |difference| / |gradient|_2: KUKA fixed base (3 x 96, nf = 2, classic) 2.2e-8, threeLinks
    floating (2 x 64, bounded) 9.9e-9 (CHAIN_MEASURED).  Bar: 10 x that, capped at 1e-4 of the gradient's norm."""
    topo, om, ic, cands = _chain_fixture(name, floating, bounded, C, T, nf, 7)
    n, nh = topo.num_dofs, max(nf)
    reg, scale, eps, freq = 1e-4, 0.5, 1e-7, 50.0
    t = np.arange(T) / freq
    worst = 0.0
    for cand in cands:
        g, delta0 = cpu_gradient_assembly(om, cand, n, t, floating, ic, reg, scale, eps)

        def F(cd):
            Y = om.regressor(_states_of(cd, n, t, floating))[:, ic]
            return -scale * np.linalg.slogdet(Y.T @ Y + delta0 * np.eye(ic.size))[1]

        def moved(key, idx, h):
            cd = {k_: (v.copy() if isinstance(v, np.ndarray) else v) for k_, v in cand.items()}
            if key == "wf":
                cd["wf"] = cand["wf"] + h
            else:
                cd[key][idx] += h
            return cd

        jl = n - 1  # (a joint with nf = 2 in both fixtures)
        coords = [("wf", None, 0), ("q_offset", 1, 1 + 1), ("a", (0, 0), 1 + 2 * n), ("a", (jl, 1), 1 + 2 * n + jl * nh + 1),
                  ("b", (0, 1), 1 + 2 * n + n * nh + 1), ("b", (jl, 0), 1 + 2 * n + n * nh + jl * nh)]
        gn = np.linalg.norm(g)
        for key, idx, e in coords:
            h = 1e-3
            D = [(F(moved(key, idx, hh)) - F(moved(key, idx, -hh))) / (2 * hh) for hh in (h, h / 2)]
            rich = (4 * D[1] - D[0]) / 3
            worst = max(worst, abs(g[e] - rich) / gn)
            assert abs(rich) > 1e-6 * gn or key == "wf", (key, idx)  # (the coordinate carries signal)
    print("chain mathematics", name, "worst |assembled - Richardson| / |g|:", worst)
    assert worst <= min(10 * CHAIN_MEASURED[name], 1e-4)


def test_subsampled_assembly_approximates_the_full_gradient():
    """subsample = k sweeps every k-th sample and scales by k (analyticalGradientSubsample): a Riemann sum of the same integrand, so it stays
    near the full gradient (here 20 % of its norm at k = 2 on a smooth 96-sample trajectory) -- a wrong or missing factor k is 50 %."""
    topo, om, ic, cands = _chain_fixture("kuka_lwr4", False, False, 1, 96, [2] * 7, 7)
    t = np.arange(96) / 50.0
    g1, _ = cpu_gradient_assembly(om, cands[0], 7, t, False, ic, 1e-4, 0.5, 1e-7)
    g2, _ = cpu_gradient_assembly(om, cands[0], 7, t, False, ic, 1e-4, 0.5, 1e-7, subsample=2)
    assert np.linalg.norm(g2 - g1) <= 0.2 * np.linalg.norm(g1)
