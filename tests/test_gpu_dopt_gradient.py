"""D-optimality gradient of candidate trajectories on the device: fbr_regressor_weights against einsum(regressor, C), fbr_fourier_gradient
against the longdouble restatement (tests/fourier_gradient_restatement.py), and excitation.candidate_dopt_gradient_from_coefficients
against the same pipeline assembled on the CPU from oracle regressors."""
import numpy as np
import pytest

import fourier_gradient_restatement as fgr
from common import load_topo, random_states

pytestmark = pytest.mark.gpu


def _engine(name, floating, friction):
    from flobaroid_amd._lib import Engine

    topo = load_topo(name)
    return topo, Engine(topo, floating=bool(floating), friction=bool(friction))


def _states(topo, eng, S, seed):
    st = random_states(topo, S, np.random.default_rng(seed), eng.floating, use_limits=True)
    if eng.friction:
        st["sign"] = np.tanh(st["dq"] / 0.02)
    return st


def _to_device(st):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in st.items()}


# (robot, floating, friction, samples, groups, selected columns: None = all, int = that many sorted random ones)
WEIGHT_CASES = [
    ("threeLinks", 0, 0, 37, 1, 11),
    ("kuka_lwr4", 0, 1, 30, 5, 43),
    ("walkman_left_arm", 1, 1, 24, 2, 50),
    ("walkman_apriori", 1, 0, 21, 3, 213),  # T = 7: 245 rows per group, tiles of 32 rows straddle; 213 = 13 * 16 + 5 = 53 * 4 + 1
    ("walkman_apriori", 1, 0, 21, 1, 213),
    ("walkman_apriori", 1, 0, 6, 2, None),  # all 480 columns: one 16-row sub-tile per workgroup
    ("kuka_lwr4", 0, 0, 19, 1, 1),
]


@pytest.mark.parametrize("case", WEIGHT_CASES, ids=lambda c: f"{c[0]}-fb{c[1]}-fr{c[2]}-S{c[3]}-g{c[4]}-c{c[5]}")
def test_regressor_weights_match_einsum(case):
    """Bar 1e-11 * max|Y C| (the project's bar for fbr_fd_scores).  C is random and unsymmetric (a transposed operand fails), the output
    starts as NaN: unselected columns must come back as exact 0.0, selected ones finite; two calls give the same bits; the host path and a
    pass cut into 5-sample chunks (tiles then start inside groups) give those bits too."""
    import torch

    name, fb, fr, S, ng, sel = case
    topo, eng = _engine(name, fb, fr)
    rng = np.random.default_rng(S + 7 * ng)
    st = _states(topo, eng, S, 3)
    P, rows = eng.cols, eng.rows
    cols = None if sel is None else np.sort(rng.choice(P, sel, replace=False)).astype(np.int32)
    nc = P if cols is None else sel
    C = rng.standard_normal((ng, nc, nc))
    Y = eng.regressor(st).reshape(ng, -1, P)
    want = np.zeros_like(Y)
    ci = np.arange(P) if cols is None else cols
    want[:, :, ci] = np.einsum("grk,gkj->grj", Y[:, :, ci], C)
    want = want.reshape(S * rows, P)
    dst = _to_device(st)
    out = torch.full((S * rows, P), float("nan"), dtype=torch.float64, device="cuda")
    got = eng.regressor_weights(dst, ng, C, cols=cols, out=out).cpu().numpy()
    assert np.all(np.isfinite(got))
    unsel = np.setdiff1d(np.arange(P), ci)
    assert np.all(got[:, unsel] == 0.0) and not np.any(np.signbit(got[:, unsel]))
    err = np.abs(got - want).max()
    print("regressor_weights", case, "err", err, "bar", 1e-11 * np.abs(want).max())
    assert err <= 1e-11 * np.abs(want).max()
    again = eng.regressor_weights(dst, ng, torch.from_numpy(C).cuda(), cols=cols).cpu().numpy()
    assert np.array_equal(got, again)
    host = eng.regressor_weights(st, ng, C, cols=cols, out=np.full((S * rows, P), np.nan))
    assert np.array_equal(got, host)
    eng.set_option("chunk_samples", 5)
    assert np.array_equal(got, eng.regressor_weights(dst, ng, C, cols=cols).cpu().numpy())
    eng.close()


def test_regressor_weights_edge_cases():
    from flobaroid_amd._lib import FbrError

    topo, eng = _engine("threeLinks", 0, 0)
    st = _states(topo, eng, 10, 1)
    C = np.zeros((3, eng.cols, eng.cols))
    with pytest.raises(FbrError, match="multiple of ngroups"):
        eng.regressor_weights(st, 3, C)
    with pytest.raises(FbrError, match="cols"):
        eng.regressor_weights(st, 1, np.zeros((1, 2, 2)), cols=[1, 1])
    empty = {k: v[:0] for k, v in st.items()}
    assert eng.regressor_weights(empty, 1, C[:1]).shape == (0, eng.cols)
    eng.close()


@pytest.mark.parametrize("bounded", [False, True], ids=["classic", "bounded"])
@pytest.mark.parametrize("nharm", [1, 6])
def test_fourier_gradient_matches_longdouble_restatement(bounded, nharm):
    """Per entry: 1e-12 * max(1, largest phase) * sum_t |terms| (a sum of T <= 2048 products carries T eps = 2.3e-13 of it; the phase
    rounding eps x is what sincos sees).  T crosses the 64-sample block of the kernel; the bits repeat."""
    import torch

    topo, eng = _engine("kuka_lwr4", 0, 0)
    n, freq = eng.n, 50.0
    rng = np.random.default_rng(17 + nharm + bounded)
    worst = 0.0
    for C in (1, 5):
        for T in (1, 63, 64, 65, 200):
            for ts in (1, 3):
                nf = rng.integers(1, nharm + 1, n)
                nf[0] = nharm
                A, B = rng.uniform(-0.5, 0.5, (C, n, nharm)), rng.uniform(-0.5, 0.5, (C, n, nharm))
                for j in range(n):  # ragged: harmonics beyond a joint's own are zero coefficients
                    A[:, j, nf[j]:] = 0.0
                    B[:, j, nf[j]:] = 0.0
                wf = 2 * np.pi * rng.uniform(0.05, 0.2, C)
                qr = rng.uniform(0.2, 1.5, (C, n)) if bounded else None
                sens = rng.standard_normal((3, C * T, n))
                got = eng.fourier_gradient(wf, A, B, sens[0], sens[1], sens[2], T, freq, q_range=qr, tstride=ts)
                dev = [torch.from_numpy(s.copy()).cuda() for s in sens]
                on_dev = eng.fourier_gradient(wf, A, B, dev[0], dev[1], dev[2], T, freq, q_range=qr, tstride=ts)
                assert np.array_equal(got, on_dev.cpu().numpy())
                assert np.array_equal(got, eng.fourier_gradient(wf, A, B, sens[0], sens[1], sens[2], T, freq, q_range=qr, tstride=ts))
                t = (np.arange(T) * ts).astype(np.longdouble) / np.longdouble(freq)
                for c in range(C):
                    s = [x.reshape(C, T, n)[c] for x in sens]
                    want, mag = fgr.chain(wf[c], None if qr is None else qr[c], A[c], B[c], s[0], s[1], s[2], t)
                    phase = max(1.0, float(wf[c] * nharm * t[-1]))
                    err = np.abs(got[c].astype(np.longdouble) - want)
                    bar = 1e-12 * phase * mag
                    worst = max(worst, float((err / np.maximum(bar, np.finfo(float).tiny)).max()))
                    assert np.all(err <= bar), (C, T, ts, c, int(np.argmax(err - bar)), float(err.max()))
                    if not bounded:
                        assert np.all(got[c, 1 + n:1 + 2 * n] == 0.0)
    print("fourier_gradient worst err / bar:", worst)
    eng.close()


def _independent_columns(eng, topo, seed=1):
    import scipy.linalg as sla

    st = random_states(topo, 2000, np.random.default_rng(seed), eng.floating, use_limits=True)
    if eng.friction:
        st["sign"] = np.tanh(st["dq"] / 0.02)
    R, piv = sla.qr(eng.gram(st), pivoting=True, mode="r")
    d = np.abs(np.diag(R))
    return np.sort(piv[: int(np.sum(d > 1e-9 * d[0]))])


def _random_candidates(topo, n, C, nh, bounded, rng):
    from flobaroid_amd import excitation as exc

    lim = [(topo.limits[j]["lower"], topo.limits[j]["upper"]) for j in topo.dof_names] if bounded else None
    cands, nf = [], rng.integers(1, nh + 1, n)
    nf[0] = nh
    for _ in range(C):
        a = [rng.uniform(-0.3, 0.3, k) for k in nf]
        b = [rng.uniform(-0.3, 0.3, k) for k in nf]
        cands.append(exc.fourier_coefficients(a, b, rng.uniform(-0.05, 0.05, n), nf, 2 * np.pi * rng.uniform(0.08, 0.12), joint_limits=lim))
    return cands


@pytest.mark.parametrize("name,floating,C,T,k,bounded,friction", [("kuka_lwr4", 0, 3, 96, 1, False, 0), ("walkman_apriori", 1, 2, 70, 3, True, 0),
                                                                  ("kuka_lwr4", 0, 2, 48, 1, False, 1)],
                         ids=["kuka-3x96", "walkman-fb-2x70-sub3", "kuka-friction-2x48"])
def test_candidate_dopt_gradient_matches_cpu_assembly(name, floating, C, T, k, bounded, friction):
    """The device pipeline against the same forward difference (eps = 1e-7) of oracle regressors with the same C, chained by the
    restatement.  Per-sensitivity bar 1e-10 * max|score| / eps (the bar of test_dopt_sensitivities_match_the_reference_worker), an entry's
    bar = that chained through sum_t |d series|.  One candidate per chunk returns the same bits; f is candidate_dopt_from_coefficients."""
    from flobaroid_amd import excitation as exc
    from oracle.oracle import OracleModel

    topo, eng = _engine(name, floating, friction)
    n, rows, P = eng.n, eng.rows, eng.cols
    rng = np.random.default_rng(23)
    freq, eps, nh = 50.0, 1e-7, 2
    cands = _random_candidates(topo, n, C, nh, bounded, rng)
    ic = _independent_columns(eng, topo)
    f, grad = exc.candidate_dopt_gradient_from_coefficients(eng, cands, T, freq, ic, dopt_scale=0.5, epsilon=eps, subsample=k)
    f1, grad1 = exc.candidate_dopt_gradient_from_coefficients(eng, cands, T, freq, ic, dopt_scale=0.5, epsilon=eps, subsample=k,
                                                              max_weight_bytes=1)
    assert np.array_equal(f, f1) and all(np.array_equal(grad[key], grad1[key]) for key in grad)
    assert np.array_equal(f, 0.5 * exc.candidate_dopt_from_coefficients(eng, cands, T, freq, ic))
    # the same pipeline on the CPU
    st = exc.candidate_states(eng, cands, T, freq, device=False)
    if friction:  # the Coulomb column tanh(dq / 0.02), held at its baseline value through the sweep
        st["sign"] = np.tanh(st["dq"] / 0.02)
    Cm, cols = exc.dopt_weight_matrices(eng.gram_grouped(st, C), ic, 1e-4, 0.5)
    om = OracleModel(topo, floating=bool(floating), fric=bool(friction))
    Ts = (T + k - 1) // k
    sub = {key: v.reshape(C, T, -1)[:, ::k].reshape(C * Ts, -1) for key, v in st.items()}
    S = C * Ts
    Y0 = om.regressor(sub, sign=sub.get("sign")).reshape(C, Ts * rows, P)
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
            sc = np.einsum("sx,sx->s", W, om.regressor(pert, sign=sub.get("sign")).reshape(S, rows * P))
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
    print("candidate_dopt_gradient", name, "worst err / bar:", worst)
    eng.close()
