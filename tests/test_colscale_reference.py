"""The column-scaled bars of tests/colscale.py, pinned on the reference alone (no GPU): these conditions keep the device bars of
tests/test_gpu_colscale.py from going slack.  The printed figures are the CPU table of DESIGN.md 2 ("Column-scaled bars")."""
import numpy as np
import pytest

import colscale as cs
import edge_reference as er

LD = np.longdouble
FLOATING = [k for k in er.CONFIG_KEYS if er.config(k)[1]]
SENSITIVE = ("ordinary", "fast", "hardacc")


def test_metric_floors_regressor_columns_and_leaves_rhs_columns_alone():
    """d = (1, 1e-3, 1e-8 | 1e-9, 0): at theta = 1e-2 the two small regressor columns are judged at 1e-2, the rhs column on its own 1e-9,
    and the zero rhs column is not used."""
    d = np.array([1.0, 1e-3, 1e-8, 1e-9, 0.0], dtype=LD)
    Gref = np.diag(d * d)
    dt = cs.column_scales(Gref, 3, 1e-2)
    assert np.allclose(np.asarray(dt[:4], dtype=float), [1.0, 1e-2, 1e-2, 1e-9], rtol=1e-15) and dt[4] == 0
    for (i, j), scale in {(0, 0): 1.0, (1, 1): 1e-4, (2, 1): 1e-4, (3, 3): 1e-18, (3, 0): 1e-9}.items():
        G = Gref.copy()
        G[i, j] += LD(1e-12) * LD(scale)
        assert abs(cs.metric(G, Gref, 1e-2, 3) / 1e-12 - 1) < 1e-6, (i, j)
    G = Gref.copy()
    G[4, 2] = 1.0
    assert cs.metric(G, Gref, 1e-2, 3) == 0.0               # a zero rhs column is not used
    assert cs.metric(Gref, Gref, 0.0, 3) == 0.0
    G = Gref.copy()
    G[2, 2] *= 1 + LD(1e-12)
    assert abs(cs.metric(G, Gref, 0.0, 3) / 1e-12 - 1) < 1e-6 and cs.metric(G, Gref, 1e-2, 3) < 2e-24  # (the floor hides it)


@pytest.mark.parametrize("key", er.CONFIG_KEYS)
def test_cpu_routes_stay_under_their_caps(key):
    """Every CPU route -- the double oracle, the emulation of the kernels' regressor, the emulation's reduced robots expanded through E,
    and for a factor LAPACK's Householder R -- on the inputs of every call of the device test, every class, both sizes:
    m_1e-2 <= 1.5e-14 and m_1e-4 <= 2.5e-13 for a class's own 24 samples (colscale.cap adds the worst-case N u of the rows beyond them
    for the tiled and the merged calls).  A route that leaves a cap fails here; the device's bar does not grow with it."""
    worst = {}
    table = {}
    over = []
    for what, calls in cs.device_calls(key).items():
        for label, call in calls:
            for route, m in cs.cpu_metrics(key, call).items():
                name = "reduced" if route.startswith("reduced") else route
                for th in cs.THETAS:
                    worst[(name, th)] = max(worst.get((name, th), 0.0), m[th])
                    if what in ("gram k=0 S=24", "tsqr S=24"):
                        table[(name, th)] = max(table.get((name, th), 0.0), m[th])
                    if m[th] > cs.cap(key, call)[th]:
                        over.append((what, label, route, th, m[th]))
    for tag, by in (("class by class at S=24 (gram k=0, tsqr)", table), ("every call of the device test", worst)):
        for name in sorted({n for n, _ in by}):
            print(f"colscale cpu | {key} | {tag} | {name} | " + " ".join(f"m_{th:g}={by[(name, th)]:.1e}" for th in cs.THETAS))
    assert not over, over


@pytest.mark.parametrize("key", er.CONFIG_KEYS)
def test_the_device_bars_are_a_hundred_times_tighter_than_the_frobenius_bar(key):
    """bar_1e-2 of a class's own 24 samples comes to about 1e-13 (16 x a few 1e-15, plus 24 x rows x 2^-53): at most 3e-13."""
    for what, calls in cs.device_calls(key).items():
        for label, call in calls:
            b = cs.bar(key, call)
            assert cs.nonzero_rows(key, call) * cs.U < b[1e-2] <= b[1e-4]
            if call.rep == 1 and len(call.classes) == 1:
                assert b[1e-2] <= 3e-13 <= er.BAR / 30, (what, label, b)


@pytest.mark.parametrize("key", er.CONFIG_KEYS)
def test_a_1e12_relative_error_in_a_small_column_passes_frobenius_and_fails_the_column_scaled_bar(key):
    """The sensitivity claim, without a GPU: the double oracle's Gram of a class, one diagonal entry -- that of the smallest column within
    100 x of the largest -- multiplied by 1 + 1e-12.  The Frobenius ratio stays below the suite's 1e-11 by more than two orders (a
    deviation 100 x larger would still pass it); m_1e-2 reads 1e-12 and is over the bar of that very call."""
    ref = er.reference(key)
    for cls in SENSITIVE:
        call = cs.Call((cls,), 1, 0)
        Gref, nY = cs.reference_gram(key, call)
        G = np.asarray(cs.cpu_grams(key, call)["oracle"], dtype=LD)
        d = np.sqrt(np.diag(Gref))
        own = np.flatnonzero(d >= LD(1e-2) * d.max())
        j = own[np.argmin(d[own])]
        before = (cs.frobenius_ratio(G, Gref), cs.metric(G, Gref, 1e-2, nY))
        G[j, j] *= 1 + LD(1e-12)
        frob, m = cs.frobenius_ratio(G, Gref), cs.metric(G, Gref, 1e-2, nY)
        print(f"colscale mutation | {key} | {cls} | column {j} of {ref['P']}, d_j / d_max = {float(d[j] / d.max()):.1e} | "
              f"frobenius {before[0]:.1e} -> {frob:.1e} | m_1e-2 {before[1]:.1e} -> {m:.1e} | bar {cs.bar(key, call)[1e-2]:.1e}")
        assert frob <= er.BAR / 100, (key, cls, frob)
        assert 0.99e-12 <= m <= 1.01e-12, (key, cls, m)
        assert before[1] <= cs.CAP[1e-2] and m > cs.bar(key, call)[1e-2], (key, cls)


def test_noise_columns_of_a_fixed_base_need_the_floor():
    """kuka_lwr4, fixed base: 20 of 108 columns are exactly zero in the long-double reference and more are rounding residue of 1e-20 of
    the largest; in double they are 1e-17-sized noise, and without a floor the oracle itself reads above 1.  With theta = 1e-2 it stays
    under its cap.  The floating-base configurations need no floor: the oracle stays at 1e-13 at theta = 0."""
    key = "kuka-fric-st0.05"
    call = cs.Call(("ordinary",), 1, 0)
    Gref, nY = cs.reference_gram(key, call)
    d = np.sqrt(np.diag(Gref))
    assert nY == 108 and int((d == 0).sum()) == 20
    assert int(((d > 0) & (d < LD(1e-18) * d.max())).sum()) >= 1
    G = cs.cpu_grams(key, call)["oracle"]
    m0 = cs.metric(G, Gref, 0.0, nY)
    print(f"colscale noise | {key} | ordinary | m_0 = {m0:.1e} | m_1e-2 = {cs.metric(G, Gref, 1e-2, nY):.1e}")
    assert m0 > 1.0 and cs.metric(G, Gref, 1e-2, nY) <= cs.CAP[1e-2]
    for fkey in FLOATING:
        for cls in er.reference(fkey)["names"]:
            call = cs.Call((cls,), 1, 0)
            Gref, nY = cs.reference_gram(fkey, call)
            m0 = cs.metric(cs.cpu_grams(fkey, call)["oracle"], Gref, 0.0, nY)
            assert m0 <= 2.5e-13, (fkey, cls, m0)


@pytest.mark.parametrize("key", FLOATING)
def test_long_double_householder_reproduces_the_reference_gram(key):
    """m_0(R^T R) <= 1e-17 for the long-double Householder factor of [Y_ref | rhs], on every entry's own scale and without a floor; with
    pivoting the same Gram comes back in the pivot order."""
    ref = er.reference(key)
    idx = cs._rows_of(key, ("ordinary",))
    A = np.concatenate([ref["Y"].reshape(-1, ref["P"])[idx], np.asarray(cs.inputs(key)["rhs"].reshape(-1, 2)[idx], dtype=LD)], axis=1)
    Gref, nY = cs.reference_gram(key, cs.Call(("ordinary",), 1, 2))
    R = cs.householder_ld(A)
    assert R.dtype == LD and np.all(np.tril(R, -1) == 0)
    m0 = cs.metric(cs.rtr(R), Gref, 0.0, nY)
    print(f"colscale householder | {key} | m_0(R^T R) = {m0:.1e}")
    assert m0 <= 1e-17
    Rp, order = cs.householder_ld(A[:, :nY], pivot=True)
    assert sorted(order) == list(range(nY)) and cs.metric(cs.rtr(Rp), Gref[np.ix_(order, order)], 0.0, nY) <= 1e-17
    diag = np.abs(np.diag(Rp))
    assert np.all(diag[1:] <= diag[:-1] * (1 + LD(1e-15)))
    rng = np.random.default_rng(3)
    x = np.asarray(rng.standard_normal(9), dtype=LD)
    Rw = np.asarray(np.triu(rng.standard_normal((9, 9))) + 4 * np.eye(9), dtype=LD)
    assert np.abs(cs.back_substitute(Rw, Rw @ x) - x).max() <= 1e-17


@pytest.mark.parametrize("key", cs.LS_KEYS)
def test_least_squares_tells_a_householder_factor_from_a_cholesky_factor(key):
    """The preconditions of the device's least-squares test: LAPACK's QR of the oracle's double matrix solves every case to 1e-11 of the
    long-double solution, and normal equations + Cholesky in double are at least 100 x worse in the fast and hard-acceleration classes --
    so 16 x e_qr passes a QR and fails a Cholesky-quality factor."""
    want = {"walkman_left_arm-fb-fric": 80, "tree12-fb": 70}[key]
    for cls in cs.LS_CLASSES:
        ls = cs.ls_case(key, cls)
        print(f"colscale least squares | {key} | {cls} | {ls['cols'].size} independent columns | e_qr = {ls['e_qr']:.1e} | e_chol = {ls['e_chol']:.1e}")
        assert ls["cols"].size == want, (key, cls, ls["cols"].size)
        assert ls["e_qr"] <= 1e-11, (key, cls, ls["e_qr"])
        if cls != "ordinary":
            assert ls["e_chol"] >= 100 * ls["e_qr"], (key, cls, ls["e_qr"], ls["e_chol"])
