"""The 50-digit reference of the observability analysis (mpmath ``eigsy`` with vectors), the matrix families the emulation and the device
are held on, and the bars (tests/test_dopt_observability.py, tests/test_gpu_dopt_observability.py).

Reference, per candidate: M = the lower triangle of G[cols, cols] (+ prior) mirrored; eigenpairs at 50 digits; lm = max(ev_max, 0), cut =
threshold^2 lm; index i is unobservable iff max(ev_i, 0) < cut; energy[j] = sum of V[j][i]^2 over those i; n_observable; margin = min_i
|ev_i - cut| / cut (inf when cut = 0); gap = the distance between the last unobservable and the first observable eigenvalue (inf when
either set is empty).  Seconds of mpmath per matrix at n = 64, so every family with n >= 24 is kept with its matrices and its reference
under tests/golden/dopt_obs (``python tests/dopt_obs_reference.py`` writes the files); the small ones are computed once per process.

Families: those of dopt_reference.py, each with a threshold that keeps its spectrum clear of the cut (``THRESHOLDS``; 1e-6, the
reference's default, where nothing else is said), plus, at n in SIZES = 1, 2, 3, 5, 24, 63, 64, 65 (either side of the 64-lane step):
  ``obs{n}``: candidates, as far as n holds them, with exact null spaces of dimension 1, 3 and n / 2 (Y of small integers with zero
      columns and columns that are twice another, Gram in long double, hence exact: a pair of EQUAL columns would put the scores on 0.5
      itself, so the copies are doubled and the scores are 0.8 / 0.2), a cluster of 8 eigenvalues spread over 1e-14 lambda_max at twice
      the cut (n >= 24), and one eigenvalue at cut (1 + 0.5) / cut (1 - 0.5);
  ``band{n}`` (n >= 2): one eigenvalue on the cut itself, inside the band: expects status bit 4 and nothing else;
  ``zero1``, and ``zero`` of the old families: nothing is unobservable.

Bars (none is fixed in advance; each is LAPACK's own figure on the same inputs, as dopt_reference.bar_lambda):
  residual  max_i |M v_i - eig_i v_i|_2 / |M|_2 (long double products): the worst of ``numpy.linalg.eigh``'s vectors against the
            reference eigenvalues over the families, by size class, x 16, floored at n eps;
  orthogonality  max |V^T V - I|: the same;
  energy    Davis-Kahan: 2 bar_lambda(n) lambda_max / gap + n eps.
LAPACK_WORST_OBS holds the measured figures (asserted by test_dopt_observability.py::test_lapack_figures_the_bars_are_built_from):

  size class   eigh residual   eigh orthogonality   emulation = device (the same bits): worst fraction of the bar (residual, orthogonality, energy)
  n <= 8       5.21e-16        1.89e-15             0.071, 0.080, 0.021
  n <= 32      7.93e-16        2.66e-15             0.100, 0.118, 0.007
  n <= 65      1.45e-15        2.89e-15             0.085, 0.388, 0.011

Conditions on the inputs, asserted here (``check_conditions``): outside the band families no reference eigenvalue within 10 band(n)
lambda_max of the cut; gap >= 1e-6 lambda_max; no score within 10 x the energy bar of 0.5."""
import functools
import os

import mpmath as mp
import numpy as np

import dopt_reference as dr

EPS = dr.EPS
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dopt_obs")
SIZES = (1, 2, 3, 5, 24, 63, 64, 65)
THRESHOLDS = {"logspace5": 3e-3, "logspace24": 3e-3, "logspace63": 3e-3, "logspace64": 3e-3, "logspace65": 3e-3, "clusters": 1e-2,
              "near_delta": 1e-3}
_NEW_THRESHOLD = 1e-2  # of obs{n} and band{n}: cut = 1e-4 lambda_max
_REF_KEYS = ("ev", "energy", "n_observable", "margin", "gap")
# worst figures of numpy.linalg.eigh over the families by size class, rounded up: (residual, orthogonality)
LAPACK_WORST_OBS = {8: (5.3e-16, 1.9e-15), 32: (8.0e-16, 2.7e-15), 65: (1.5e-15, 2.9e-15)}


def band(n):
    """band(n) of csrc/fbr_dopt.h: what fp64 knows of an eigenvalue of the Gram, relative to lambda_max"""
    return max(128, n) * EPS


assert all(band(n) >= dr.bar_lambda(n) for n in range(1, 513))


def _class(n):
    return min([k for k in LAPACK_WORST_OBS if n <= k] or [65])


def bar_residual(n):
    return max(16.0 * LAPACK_WORST_OBS[_class(n)][0], n * EPS)


def bar_orthogonality(n):
    return max(16.0 * LAPACK_WORST_OBS[_class(n)][1], n * EPS)


def bar_energy(n, ref):
    return (2.0 * dr.bar_lambda(n) * abs(ref["ev"][-1]) / ref["gap"] if np.isfinite(ref["gap"]) else 0.0) + n * EPS


def mp_reference(M, thr):
    with mp.workdps(50):
        n = M.shape[0]
        if n == 1:
            ev, V = [mp.mpf(float(M[0, 0]))], [[mp.mpf(1)]]
        else:
            E, Q = mp.eigsy(mp.matrix(M.tolist()))
            order = sorted(range(n), key=lambda i: E[i])
            ev = [E[i] for i in order]
            V = [[Q[j, i] for i in order] for j in range(n)]
        lm = max(ev[-1], mp.mpf(0))
        cut = mp.mpf(thr) * mp.mpf(thr) * lm
        un = [i for i in range(n) if max(ev[i], mp.mpf(0)) < cut]
        ob = [i for i in range(n) if i not in un]
        energy = [float(sum(V[j][i] ** 2 for i in un)) for j in range(n)]
        margin = float(min(abs(e - cut) / cut for e in ev)) if cut > 0 else float("inf")
        gap = float(min(ev[i] for i in ob) - max(ev[i] for i in un)) if un and ob else float("inf")
        return {"ev": np.array([float(e) for e in ev]), "energy": np.array(energy), "n_observable": n - len(un), "margin": margin, "gap": gap}


def _int_null(n, kind, rng):
    """Gram of an integer Y (3 n + 2 rows) with an exact null space: 'null1': column 1 = 2 column 0 (a zero column at n = 1); 'null3': a
    zero column and two doubled copies; 'half': column 2 i + 1 = 2 column 2 i for every pair"""
    Y = rng.integers(-8, 9, size=(3 * n + 2, n)).astype(np.float64)
    if kind == "null1":
        if n == 1:
            Y[:, 0] = 0
        else:
            Y[:, 1] = 2 * Y[:, 0]
    elif kind == "null3":
        Y[:, n - 1] = 0
        Y[:, 1] = 2 * Y[:, 0]
        Y[:, 3] = 2 * Y[:, 2]
    else:
        for i in range(n // 2):
            Y[:, 2 * i + 1] = 2 * Y[:, 2 * i]
    Yl = Y.astype(np.longdouble)
    M = (Yl.T @ Yl).astype(np.float64)
    assert np.array_equal(M, M.T)
    return M


def _obs_family(n, rng):
    cut = _NEW_THRESHOLD ** 2
    if n == 1:
        return [np.array([[3.0]])]
    Ms = [_int_null(n, "null1", rng)]
    if n >= 5:
        Ms += [_int_null(n, "null3", rng), _int_null(n, "half", rng)]
    top = lambda k: list(np.logspace(0, -2, k))  # noqa: E731  (observable, well above the cut)
    if n >= 24:
        cl = [2 * cut + 1e-14 * i / 7 for i in range(8)]
        Ms.append(dr._spectrum(top(n - 11) + cl + [1e-6, 1e-7, 1e-9], rng))
    low = [1e-7, 1e-9][: max(0, n - 2)]
    for f in (1.5, 0.5):
        Ms.append(dr._spectrum(top(n - 1 - len(low)) + [cut * f] + low, rng))
    return Ms


def _band_family(n, rng):
    cut = _NEW_THRESHOLD ** 2
    low = [1e-7][: max(0, n - 2)]
    return [dr._spectrum(list(np.logspace(0, -2, n - 1 - len(low))) + [cut] + low, rng)]


def families():
    """name -> (list of M, threshold, prior or None)"""
    f = {name: (Ms, THRESHOLDS.get(name, 1e-6), prior) for name, (Ms, _, prior, _) in dr.families().items()}
    rng = np.random.default_rng(29)
    f["zero1"] = ([np.zeros((1, 1))], 1e-6, None)
    for n in SIZES:
        f[f"obs{n}"] = (_obs_family(n, rng), _NEW_THRESHOLD, None)
        if n >= 2:
            f[f"band{n}"] = (_band_family(n, rng), _NEW_THRESHOLD, None)
    for name in list(f):  # the stored matrices take the place of the generated ones
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        if os.path.exists(path):
            with np.load(path) as z:
                f[name] = (list(z["Ms"]),) + f[name][1:]
    return f


@functools.lru_cache(maxsize=None)
def _families():
    return families()


CASES = list(families())
BAND_CASES = [c for c in CASES if c.startswith("band")]


def is_golden(name):
    return _families()[name][0][0].shape[0] >= 24


@functools.lru_cache(maxsize=None)
def case(name):
    """(G, cols, threshold, prior) of a family: the matrices embedded as dopt_reference.embed embeds them"""
    Ms, thr, prior = _families()[name]
    G, cols = dr.embed(Ms, prior, np.random.default_rng(sum(map(ord, name))))
    return G, cols, thr, prior


def _lapack_figures(M, ev_ref):
    """(residual, orthogonality) of numpy.linalg.eigh's vectors, the residual against the reference eigenvalues"""
    n = M.shape[0]
    _, V = np.linalg.eigh(M)
    return residual(M, ev_ref, V), float(np.abs(V.T @ V - np.eye(n)).max())


def residual(M, eig, V):
    nm = np.linalg.norm(M, 2)
    if nm == 0:
        return 0.0
    Ml, Vl = M.astype(np.longdouble), V.astype(np.longdouble)
    R = Ml @ Vl - Vl * eig.astype(np.longdouble)
    return float(np.sqrt((R * R).sum(axis=0)).max() / nm)


@functools.lru_cache(maxsize=None)
def reference(name):
    """list (one per candidate) of mp_reference dicts of a family, each with "M" and numpy.linalg.eigh's own figures"""
    G, cols, thr, prior = case(name)
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    stored = dict(np.load(path)) if os.path.exists(path) else None
    assert stored is not None or not is_golden(name), (name, "its reference is missing under tests/golden/dopt_obs")
    out = []
    for c in range(G.shape[0]):
        M = dr.lower_mirrored(G[c], cols, prior)
        if stored is not None:
            assert np.array_equal(stored["Ms"][c] + (0 if prior is None else prior), M), (name, "the stored matrix is not the one the case feeds")
            r = {k: (stored[k][c].item() if stored[k][c].ndim == 0 else stored[k][c]) for k in _REF_KEYS}
        else:
            r = mp_reference(M, thr)
        r["M"] = M
        r["lapack_residual"], r["lapack_orthogonality"] = _lapack_figures(M, r["ev"])
        out.append(r)
    return out


def check_conditions(name):
    """the conditions on the inputs: a family that fails one is replaced, never its bar"""
    G, cols, thr, _ = case(name)
    n = len(cols)
    for c, r in enumerate(reference(name)):
        lm = max(r["ev"][-1], 0.0)
        cut = thr * thr * lm
        near = np.abs(r["ev"] - cut).min()
        if name in BAND_CASES:
            assert near < 0.5 * band(n) * lm, (name, c, near / lm)
            continue
        assert lm == 0 or near > 10 * band(n) * lm, (name, c, "a reference eigenvalue within 10 band of the cut", near / lm)
        assert r["gap"] >= 1e-6 * lm, (name, c, "gap", r["gap"] / lm)
        assert np.abs(r["energy"] - 0.5).min() > 10 * bar_energy(n, r), (name, c, "a score within 10 bars of 0.5")


def check_against_reference(name, got, where=""):
    """hold the dict of Engine.dopt_observability / the emulation (NumPy arrays, with eig and vec) to the bars on a family; returns the
    worst figure / bar of each quantity"""
    G, cols, thr, prior = case(name)
    n = len(cols)
    worst = {"residual": 0.0, "orthogonality": 0.0, "energy": 0.0}
    for c, r in enumerate(reference(name)):
        V, eig = got["vec"][c], got["eig"][c]
        lm = abs(r["ev"][-1])
        assert np.abs(eig - r["ev"]).max() <= dr.bar_lambda(n) * lm, (where, name, c)
        res, orth = residual(r["M"], eig, V), float(np.abs(V.T @ V - np.eye(n)).max())
        worst["residual"] = max(worst["residual"], res / bar_residual(n))
        worst["orthogonality"] = max(worst["orthogonality"], orth / bar_orthogonality(n))
        assert res <= bar_residual(n), (where, name, c, "residual", res, bar_residual(n))
        assert orth <= bar_orthogonality(n), (where, name, c, "orthogonality", orth, bar_orthogonality(n))
        big = np.argmax(np.abs(V), axis=0)  # (the first of the largest)
        assert np.all(V[big, np.arange(n)] > 0), (where, name, c, "sign")
        if name in BAND_CASES:
            assert int(got["status"][c]) == 4, (where, name, c, int(got["status"][c]))
            continue
        assert int(got["status"][c]) == 0, (where, name, c, int(got["status"][c]))
        assert int(got["n_observable"][c]) == r["n_observable"], (where, name, c, int(got["n_observable"][c]), r["n_observable"])
        be = bar_energy(n, r)
        e_en = float(np.abs(got["energy"][c] - r["energy"]).max())
        worst["energy"] = max(worst["energy"], e_en / be)
        assert e_en <= be, (where, name, c, "energy", e_en, be)
        assert np.array_equal(got["energy"][c] > 0.5, r["energy"] > 0.5), (where, name, c)
        if np.isfinite(r["margin"]):
            # margin moves with the eigenvalue nearest the cut and with lambda_max: (bar_lambda lm + bar_lambda lm (1 + margin)) / cut
            bm = dr.bar_lambda(n) * (2.0 + r["margin"]) / (thr * thr) + 4 * EPS * r["margin"]
            assert abs(got["margin"][c] - r["margin"]) <= bm, (where, name, c, "margin", got["margin"][c], r["margin"], bm)
        else:
            assert got["margin"][c] == np.inf
    return worst


def write_golden():
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    for fn in os.listdir(GOLDEN_DIR):
        os.remove(os.path.join(GOLDEN_DIR, fn))
    fam = families()
    for name, (Ms, thr, prior) in fam.items():
        if Ms[0].shape[0] < 24:
            continue
        Ms = [dr.lower_mirrored(M, np.arange(M.shape[0])) for M in Ms]
        refs = [mp_reference(M if prior is None else M + prior, thr) for M in Ms]
        np.savez_compressed(os.path.join(GOLDEN_DIR, name + ".npz"), Ms=np.stack(Ms), **{k: np.stack([np.asarray(r[k]) for r in refs]) for k in _REF_KEYS})
        print(name, "written", flush=True)


if __name__ == "__main__":
    write_golden()
