"""The 50-digit reference of the D-optimality arithmetic (mpmath), the matrix families the emulation and the device are held on, and the
bars (tests/test_dopt_reference.py, tests/test_gpu_dopt_spectrum.py).

Reference: M = the lower triangle of G[cols, cols] (+ prior) mirrored; eigsy eigenvalues; delta = reg max(lambda_max, 1e-30);
neg_log_det = -sum log(max(ev + delta, 1e-300)); n_observable = #(ev > delta); Cmat = -2 scale (M + delta I)^-1.  About 0.1 s at n = 24 and
1 to 2 s at n = 64, so it stays at n <= 65; every case is computed once per process (``reference``) and never modified.

Bars.  ``bar_lambda(n)``, relative to lambda_max: LAPACK's own worst error against the reference over the cases of this file
(``LAPACK_WORST``, asserted by test_dopt_reference.py::test_lapack_error_is_what_the_bars_are_built_from) times a margin of 16 -- a
different backward-stable algorithm has a bound p(n) eps |M| with another low-degree p, plus the device's own rounding of log -- floored at
n eps.  ``bar_neg_log_det``: |d log(ev + delta) / d ev| <= 1 / delta and delta moves with lambda_max, so n bar_lambda (1 / reg + 1) + 4 n eps;
for reg = 0 the factor is lambda_max / lambda_min of the reference instead (1 / reg is infinite: the finite factor asks more).
``bar_cmat``: NumPy's own error of inv(M + delta I) on that very matrix, measured against the reference, times 16, floored at n eps,
relative to max|Cmat|."""
import functools
import os

import mpmath as mp
import numpy as np

EPS = 2.0 ** -52
# the larger families (seconds of mpmath each) are kept with their reference under tests/golden/dopt: the matrices themselves are stored, so
# that the recorded reference belongs to the very bits the test feeds (python tests/dopt_reference.py writes the files)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dopt")
GOLDEN_FAMILIES = ("logspace24", "logspace63", "logspace64", "logspace65")
_REF_KEYS = ("ev", "neg_log_det", "lambda_max", "delta", "n_observable", "Cmat", "delta_gap")
# worst |eigvalsh - reference| / lambda_max over the cases below, by size class (n <= 8, n <= 32, n <= 65), rounded up
# (measured over the families: 6.37e-16 at n = 8, 6.66e-16 at n = 9, 1.05e-15 at n = 64; over the oracle Grams of ROBOTS below: 1.08e-15
# on threeLinks, n = 24, and 1.13e-15 on KUKA, n = 64); above 65 the last class stands, where the floor n eps is the larger
LAPACK_WORST = {8: 6.4e-16, 32: 1.1e-15, 65: 1.2e-15}


def lapack_worst(n):
    return LAPACK_WORST[min([k for k in LAPACK_WORST if n <= k] or [65])]


def bar_lambda(n):
    return max(16.0 * lapack_worst(n), n * EPS)


def bar_neg_log_det(n, reg, ev_ref=None):
    kappa = (1.0 / reg + 1.0) if reg > 0 else float(ev_ref[-1] / ev_ref[0])
    return n * bar_lambda(n) * kappa + 4 * n * EPS


def lower_mirrored(G, cols, prior=None):
    """M of one candidate as eigvalsh sees it"""
    cols = np.asarray(cols, dtype=np.int64)
    M = G[np.ix_(cols, cols)].copy()
    if prior is not None:
        M = M + prior
    L = np.tril(M)
    return L + np.tril(M, -1).T


def mp_reference(M, reg, scale=1.0, weights=True):
    """(ev ascending, neg_log_det, lambda_max, delta, n_observable, Cmat or None, ev as mpf) of one symmetric M at 50 digits; the
    float64 values are the correctly rounded ones"""
    with mp.workdps(50):
        n = M.shape[0]
        A = mp.matrix(M.tolist())
        ev = sorted(mp.eigsy(A, eigvals_only=True)) if n > 1 else [mp.mpf(float(M[0, 0]))]
        lmax = ev[-1]
        delta = mp.mpf(reg) * max(lmax, mp.mpf("1e-30"))
        nld = -sum(mp.log(max(e + delta, mp.mpf("1e-300"))) for e in ev)
        nobs = sum(1 for e in ev if e > delta)
        gap = min(abs(e - delta) / delta for e in ev) if delta > 0 else mp.inf
        Cm = None
        if weights and all(e + delta > 0 for e in ev):
            inv = mp.inverse(A + delta * mp.eye(n))
            Cm = np.array([[float(-2 * mp.mpf(scale) * inv[i, j]) for j in range(n)] for i in range(n)])
        return {"ev": np.array([float(e) for e in ev]), "neg_log_det": float(nld), "lambda_max": float(lmax), "delta": float(delta),
                "n_observable": int(nobs), "Cmat": Cm, "delta_gap": float(gap)}


# ---------------------------------------------------------------------------------------------------------------------------------
# matrix families: name -> (list of M (n, n), reg, prior or None, scale per candidate or None)
# ---------------------------------------------------------------------------------------------------------------------------------
def _q(n, rng):
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


def _spectrum(ev, rng):
    Q = _q(len(ev), rng)
    M = (Q * np.asarray(ev)) @ Q.T
    return 0.5 * (M + M.T)


def _spd(n, rng):
    Y = rng.standard_normal((3 * n + 2, n))
    return Y.T @ Y


def families():
    rng = np.random.default_rng(11)
    f = {}
    for n in (1, 2, 3):
        f[f"n{n}"] = ([_spd(n, rng) for _ in range(3)], 1e-4, None, None)
    f["diagonal"] = ([np.diag([5.0, 3.0, 3.0, 2.0, 1.0, 0.5]), np.diag([7.0, 7.0, 4.0, 0.25, 0.25, 0.125])], 1e-4, None, None)
    tri = []
    for _ in range(2):
        d, e = 1.0 + rng.random(7), rng.standard_normal(6) * 0.4
        tri.append(np.diag(d) + np.diag(e, 1) + np.diag(e, -1))
    f["tridiagonal"] = (tri, 1e-4, None, None)
    f["c_identity"] = ([2.5 * np.eye(5), 1e-3 * np.eye(5)], 1e-4, None, None)
    f["zero"] = ([np.zeros((4, 4)), np.zeros((4, 4))], 1e-4, None, None)
    for n in (5, 24, 63, 64, 65):
        # (reg = 2e-4: with 1e-4 an eigenvalue of the n = 64 ladder sits on delta itself)
        f[f"logspace{n}"] = ([_spectrum(np.logspace(0, -12, n) * 1e6, rng) for _ in range(3 if n < 60 else 2)], 2e-4, None, None)
    cl = np.concatenate([c * (1.0 + 1e-14 * np.arange(3)) for c in (1.0, 1e-3, 1e-6)])
    f["clusters"] = ([_spectrum(cl, rng) for _ in range(2)], 1e-4, None, None)
    rd = []
    for _ in range(2):
        Y = rng.standard_normal((4, 7))
        rd.append(Y.T @ Y)
    f["rank_deficient"] = (rd, 1e-4, None, None)
    dl = 1e-4
    f["near_delta"] = ([_spectrum([1.0, 0.5, 0.1, dl * (1 + 1e-3), dl * (1 - 1e-3), 1e-9], rng) for _ in range(2)], 1e-4, None, None)
    f["prior"] = ([_spd(8, rng) for _ in range(3)], 1e-4, _spd(8, rng) * 0.3, None)
    f["scale"] = ([_spd(6, rng) for _ in range(3)], 1e-3, None, np.array([0.5, 2.0, 7.25]))
    f["reg0_full_rank"] = ([_spd(6, rng) for _ in range(2)], 0.0, None, None)
    for name in GOLDEN_FAMILIES:  # the stored matrices take the place of the generated ones
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        if os.path.exists(path):
            with np.load(path) as z:
                f[name] = (list(z["Ms"]),) + f[name][1:]
    return f


@functools.lru_cache(maxsize=None)
def _families():
    return families()


CASES = list(families())


def embed(Ms, prior, rng):
    """(G (C, Pa, Pa), cols) holding the matrices at scattered columns in an order that is not sorted, Pa = n + 3 (the last column a rhs),
    the strict upper triangle of every M off by one part in 2^50 (only the lower one may be read), everything else random"""
    C, n = len(Ms), Ms[0].shape[0]
    Pa = n + 3
    cols = rng.permutation(Pa - 1)[:n].astype(np.int32)
    if n > 1 and np.all(np.diff(cols) > 0):
        cols = cols[::-1].copy()
    G = rng.standard_normal((C, Pa, Pa))
    for c, M in enumerate(Ms):
        Mu = np.tril(M) + np.triu(M, 1) * (1.0 + 4 * EPS)
        G[c][np.ix_(cols, cols)] = Mu
    return np.ascontiguousarray(G), cols


@functools.lru_cache(maxsize=None)
def case(name):
    """(G, cols, reg, prior, scale) of a family"""
    Ms, reg, prior, scale = _families()[name]
    G, cols = embed(Ms, prior, np.random.default_rng(sum(map(ord, name))))
    return G, cols, reg, prior, scale


@functools.lru_cache(maxsize=None)
def reference(name):
    """list (one per candidate) of mp_reference dicts of a family, each with "M" and NumPy's own errors"""
    G, cols, reg, prior, scale = case(name)
    out = []
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    stored = dict(np.load(path)) if name in GOLDEN_FAMILIES and os.path.exists(path) else None
    for c in range(G.shape[0]):
        M = lower_mirrored(G[c], cols, prior)
        if stored is not None:
            assert np.array_equal(stored["Ms"][c], M), (name, "the stored matrix is not the one the case feeds")
            r = {k: (stored[k][c].item() if stored[k][c].ndim == 0 else stored[k][c]) for k in _REF_KEYS}
        else:
            r = mp_reference(M, reg, 1.0 if scale is None else float(scale[c]))
        r["M"] = M
        r["lapack_err"] = float(np.abs(np.linalg.eigvalsh(M) - r["ev"]).max() / max(abs(r["lambda_max"]), 1e-300))
        if r["Cmat"] is not None:
            n = M.shape[0]
            ev = np.linalg.eigvalsh(M)
            dl = reg * max(ev[-1], 1e-30)
            inv = -2.0 * (1.0 if scale is None else float(scale[c])) * np.linalg.inv(M + dl * np.eye(n))
            r["numpy_inv_err"] = float(np.abs(inv - r["Cmat"]).max() / np.abs(r["Cmat"]).max())
        out.append(r)
    return out


def bar_cmat(n, ref):
    return max(16.0 * ref["numpy_inv_err"], n * EPS)


def check_against_reference(name, got, where=""):
    """hold the dict of Engine.dopt_terms / the emulation (NumPy arrays, with eig and Cmat) to the bars on a family; returns the worst
    error / bar of each quantity"""
    G, cols, reg, prior, scale = case(name)
    n = len(cols)
    worst = {"ev": 0.0, "nld": 0.0, "cmat": 0.0}
    for c, r in enumerate(reference(name)):
        assert r["delta_gap"] > 1e-6, (name, c, "a reference eigenvalue sits on delta")
        lm = abs(r["lambda_max"])
        e_ev = np.abs(got["eig"][c] - r["ev"]).max()
        e_lm = abs(got["lambda_max"][c] - r["lambda_max"])
        assert np.all(np.diff(got["eig"][c]) >= 0), (name, c, "eigenvalues do not ascend")
        worst["ev"] = max(worst["ev"], e_ev / (bar_lambda(n) * lm) if lm > 0 else (0.0 if e_ev == 0 else np.inf))
        assert e_ev <= bar_lambda(n) * lm and e_lm <= bar_lambda(n) * lm, (where, name, c, e_ev, e_lm, bar_lambda(n) * lm)
        want_delta = reg * max(got["lambda_max"][c], 1e-30)
        assert got["delta"][c] == want_delta, (where, name, c)
        bn = bar_neg_log_det(n, reg, r["ev"])
        e_n = abs(got["neg_log_det"][c] - r["neg_log_det"])
        worst["nld"] = max(worst["nld"], e_n / bn)
        assert e_n <= bn, (where, name, c, e_n, bn)
        assert int(got["n_observable"][c]) == r["n_observable"], (where, name, c)
        assert int(got["status"][c]) == 0
        if "Cmat" in got and r["Cmat"] is not None:
            Cm = got["Cmat"][c]
            assert np.array_equal(Cm, Cm.T), (where, name, c, "Cmat is not bit-symmetric")
            assert np.all(np.isfinite(Cm))
            e_c = np.abs(Cm - r["Cmat"]).max() / np.abs(r["Cmat"]).max()
            worst["cmat"] = max(worst["cmat"], e_c / bar_cmat(n, r))
            assert e_c <= bar_cmat(n, r), (where, name, c, e_c, bar_cmat(n, r))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# oracle Grams of the bundled robots on pivoted-QR columns, in pivot order: (robot, floating, friction, candidates, samples each)
# ---------------------------------------------------------------------------------------------------------------------------------
ROBOTS = [("threeLinks", 1, 0, 3, 40), ("kuka_lwr4", 0, 1, 2, 48), ("walkman_apriori", 1, 0, 2, 70), ("walkman_apriori", 1, 0, 2, 5)]
ROBOT_COLUMNS = {"threeLinks": 24, "kuka_lwr4": 64, "walkman_apriori": 213}


@functools.lru_cache(maxsize=None)
def oracle_grams(name, floating, friction, C, T):
    """(G (C, cols + 1, cols + 1) with a rhs column, cols in pivot order) from oracle regressors of
    random_states(topo, C * T, default_rng(5), use_limits=True)"""
    import scipy.linalg as sla
    from common import load_topo, random_states
    from oracle.oracle import OracleModel

    topo = load_topo(name)
    om = OracleModel(topo, floating=bool(floating), fric=bool(friction))

    def grams(C, T):
        st = random_states(topo, C * T, np.random.default_rng(5), bool(floating), use_limits=True)
        Y = om.regressor(st, sign=np.tanh(st["dq"] / 0.02) if friction else None)
        Y = np.concatenate([Y, np.random.default_rng(6).standard_normal((Y.shape[0], 1))], axis=1).reshape(C, -1, Y.shape[1] + 1)
        return np.einsum("crk,crj->ckj", Y, Y)

    R, piv = sla.qr(grams(1, 300)[0, :-1, :-1], pivoting=True, mode="r")
    d = np.abs(np.diag(R))
    cols = piv[: int(np.sum(d > 1e-9 * d[0]))].astype(np.int32)
    assert np.any(np.diff(cols) < 0) and len(cols) == ROBOT_COLUMNS[name]
    return grams(C, T), cols


def check_robot(case, got, scale, reg=1e-4, where=""):
    """hold the dict of Engine.dopt_terms / the emulation on oracle_grams(*case) (with ``scale`` per candidate) to the bars: against the
    reference up to n = 64; at n = 213 eigenvalues against eigvalsh at 2 bar_lambda (both sides carry that error), Cmat by both residuals
    at n eps (1 / reg + 1)"""
    name, _, _, C, T = case
    G, cols = oracle_grams(*case)
    n = len(cols)
    assert np.all(got["status"] == 0)
    for c in range(C):
        M = lower_mirrored(G[c], cols)
        Cm = got["Cmat"][c]
        ev = np.linalg.eigvalsh(M)
        assert np.array_equal(Cm, Cm.T) and np.all(np.isfinite(Cm)) and np.all(np.diff(got["eig"][c]) >= 0)
        assert got["delta"][c] == reg * got["lambda_max"][c] and got["lambda_max"][c] == got["eig"][c][-1]
        if n <= 64:
            r = mp_reference(M, reg, float(scale[c]))
            assert r["delta_gap"] > 1e-6
            lap = np.abs(ev - r["ev"]).max() / r["lambda_max"]
            assert lap <= lapack_worst(n), (name, c, lap)  # (the number the bars of this size class are built from is measured here)
            e_ev = np.abs(got["eig"][c] - r["ev"]).max() / r["lambda_max"]
            e_n = abs(got["neg_log_det"][c] - r["neg_log_det"])
            ninv = -2.0 * scale[c] * np.linalg.inv(M + reg * ev[-1] * np.eye(n))
            bar_c = max(16.0 * np.abs(ninv - r["Cmat"]).max() / np.abs(r["Cmat"]).max(), n * EPS)
            e_c = np.abs(Cm - r["Cmat"]).max() / np.abs(r["Cmat"]).max()
            print(f"{where} {name} candidate {c}: eig {e_ev:.2e} (LAPACK {lap:.2e}, bar {bar_lambda(n):.2e}), neg_log_det {e_n:.2e} "
                  f"(bar {bar_neg_log_det(n, reg):.2e}), Cmat {e_c:.2e} (bar {bar_c:.2e}), delta gap {r['delta_gap']:.2e}")
            assert e_ev <= bar_lambda(n) and e_n <= bar_neg_log_det(n, reg) and got["n_observable"][c] == r["n_observable"] and e_c <= bar_c
        else:
            lm, dl = got["lambda_max"][c], got["delta"][c]
            e_ev = np.abs(got["eig"][c] - ev).max() / ev[-1]
            assert np.min(np.abs(ev - dl) / dl) > 1e-6 and got["n_observable"][c] == int(np.sum(ev > dl))
            assert np.all(got["eig"][c] + dl > 0)
            if T == 5:  # 175 rows for 213 columns: the null space comes out as roundings of either sign
                assert got["n_observable"][c] <= 175 and np.abs(got["eig"][c][: n - 175]).max() <= 2 * bar_lambda(n) * lm
                assert got["eig"][c][0] < 0
            A = (M + dl * np.eye(n)).astype(np.longdouble)
            X = Cm.astype(np.longdouble) / np.longdouble(-2.0 * scale[c])
            res = max(float(np.abs(A @ X - np.eye(n)).max()), float(np.abs(X @ A - np.eye(n)).max()))
            print(f"{where} {name} T={T} candidate {c}: eig against eigvalsh {e_ev:.2e} (bar {2 * bar_lambda(n):.2e}), residual {res:.2e} "
                  f"(bar {n * EPS * (1 / reg + 1):.2e}), n_observable {got['n_observable'][c]}, smallest eigenvalue {got['eig'][c][0]:.2e}")
            assert e_ev <= 2 * bar_lambda(n) and res <= n * EPS * (1.0 / reg + 1.0)


def write_golden():
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    for name in GOLDEN_FAMILIES:
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        if os.path.exists(path):
            os.remove(path)
    fam = families()
    for name in GOLDEN_FAMILIES:
        Ms, reg, _, _ = fam[name]
        Ms = [lower_mirrored(M, np.arange(M.shape[0])) for M in Ms]
        refs = [mp_reference(M, reg) for M in Ms]
        np.savez_compressed(os.path.join(GOLDEN_DIR, name + ".npz"), Ms=np.stack(Ms), **{k: np.stack([np.asarray(r[k]) for r in refs]) for k in _REF_KEYS})
        print(name, "written")


if __name__ == "__main__":
    write_golden()
