"""The eigenvector / observability text of csrc/fbr_dopt.h off the GPU (g++, tests/emul/dopt_obs_emul.cpp): held to the 50-digit reference
and its bars on every matrix family (tests/dopt_obs_reference.py), the conditions on those families, LAPACK's own figures the bars are
built from, the reported eigenvalues bit for bit those of fbr_dopt_terms, refusals and the band rule, isolation of a NaN candidate; and
the host pieces: observability_fields, merge_unobservable_params, candidate_observability's mapping (against a stand-in engine)."""
import numpy as np
import pytest

import dopt_emul_lib as de
import dopt_obs_emul_lib as oe
import dopt_obs_reference as orf
import dopt_reference as dr
import observability_restatement as obr


def test_reference_on_closed_forms():
    r = orf.mp_reference(np.diag([4.0, 1.0, 1e-7, 0.0]), 1e-3)  # cut = 4e-6
    assert np.array_equal(r["ev"], [0.0, 1e-7, 1.0, 4.0]) and r["n_observable"] == 2 and np.array_equal(r["energy"], [0.0, 0.0, 1.0, 1.0])
    assert abs(r["margin"] - (4e-6 - 1e-7) / 4e-6) <= 4 * dr.EPS and abs(r["gap"] - (1.0 - 1e-7)) <= 2 * dr.EPS
    r = orf.mp_reference(np.array([[1.0, 2.0], [2.0, 4.0]]), 1e-3)  # column 1 = 2 column 0: the null vector is (2, -1) / sqrt(5)
    assert r["n_observable"] == 1 and np.abs(r["energy"] - [0.8, 0.2]).max() <= 2 * dr.EPS and abs(r["margin"] - 1.0) <= 2 * dr.EPS
    r = orf.mp_reference(np.zeros((3, 3)), 1e-3)
    assert r["n_observable"] == 3 and r["margin"] == np.inf and r["gap"] == np.inf and np.all(r["energy"] == 0.0)


def test_band_is_no_smaller_than_the_eigenvalue_bar_and_the_default_threshold_passes():
    for n in range(1, 513):
        assert oe.band(n) == orf.band(n) >= dr.bar_lambda(n)
    assert 1e-6 ** 2 >= 8 * oe.band(512)


@pytest.mark.parametrize("name", orf.CASES)
def test_conditions_on_the_inputs(name):
    orf.check_conditions(name)


def test_lapack_figures_the_bars_are_built_from():
    """numpy.linalg.eigh over every family: residual (against the reference eigenvalues) and orthogonality at most LAPACK_WORST_OBS of
    the size class, and the largest of a class within a factor of 4 of it"""
    worst = {k: [0.0, 0.0] for k in orf.LAPACK_WORST_OBS}
    for name in orf.CASES:
        n = len(orf.case(name)[1])
        for r in orf.reference(name):
            k = orf._class(n)
            worst[k][0] = max(worst[k][0], r["lapack_residual"])
            worst[k][1] = max(worst[k][1], r["lapack_orthogonality"])
    print("numpy.linalg.eigh, worst (residual, orthogonality) by size class:", worst)
    for k, (res, orth) in orf.LAPACK_WORST_OBS.items():
        assert res / 4 <= worst[k][0] <= res and orth / 4 <= worst[k][1] <= orth, (k, worst[k])


@pytest.mark.parametrize("name", orf.CASES)
def test_emulation_within_the_bars(name):
    G, cols, thr, prior = orf.case(name)
    got = oe.dopt_observability(G, cols, thr, prior=prior)
    w = orf.check_against_reference(name, got, "emulation")
    print(name, "n =", len(cols), "worst figure / bar:", {k: float(f"{v:.3g}") for k, v in w.items()})
    # the eigenvalues are bit for bit those of fbr_dopt_terms; the same bits without eig / vec and for every width of the workgroup
    assert np.array_equal(got["eig"], de.dopt_terms(G, cols, 1e-4, prior=prior, weights=False)["eig"])
    bare = oe.dopt_observability(G, cols, thr, prior=prior, eigenvalues=False, vectors=False)
    assert set(bare) == {"n_observable", "energy", "margin", "status"} and all(np.array_equal(bare[k], got[k]) for k in bare)
    for nt in (1, 256):
        other = oe.dopt_observability(G, cols, thr, prior=prior, nt=nt)
        assert all(np.array_equal(other[k], got[k]) for k in got), nt


def test_a_tie_of_the_largest_components_takes_the_first():
    got = oe.dopt_observability(np.array([[[2.0, 1.0], [1.0, 2.0]]]), [0, 1], 1e-3)
    V = got["vec"][0]  # (1, -1) / sqrt(2) for 1 and (1, 1) / sqrt(2) for 3: the first component is the positive one
    assert np.abs(got["eig"][0] - [1.0, 3.0]).max() <= 3 * dr.bar_lambda(2) and np.all(V[0] > 0) and V[1, 0] < 0
    assert abs(V[1, 0]) == V[0, 0] and V[1, 1] == V[0, 1]  # (the rotation of n = 2 has c == s: the ties are exact)


def test_large_sizes_against_lapack():
    """n = 213 and the limit n = 512 with an exact null space of dimension 2, against residual and orthogonality at the bars and the
    scores that the null vectors give exactly"""
    for n in (213, 512):
        rng = np.random.default_rng(n)
        Y = rng.integers(-8, 9, size=(2 * n, n)).astype(np.float64)
        Y[:, 5] = 0
        Y[:, 9] = 2 * Y[:, 8]
        M = Y.T @ Y
        got = oe.dopt_observability(M[None], np.arange(n), 1e-6, nt=256)
        V, eig = got["vec"][0], got["eig"][0]
        res, orth = orf.residual(M, eig, V), np.abs(V.T @ V - np.eye(n)).max()
        print(n, "residual", res, "bar", orf.bar_residual(n), "orthogonality", orth, "bar", orf.bar_orthogonality(n))
        assert res <= orf.bar_residual(n) and orth <= orf.bar_orthogonality(n)
        want = np.zeros(n)
        want[[5, 8, 9]] = [1.0, 0.8, 0.2]
        lam = np.linalg.eigvalsh(M)
        bar = 2 * dr.bar_lambda(n) * lam[-1] / lam[2] + n * dr.EPS
        assert got["n_observable"][0] == n - 2 and got["status"][0] == 0 and np.abs(got["energy"][0] - want).max() <= bar
        assert abs(got["margin"][0] - 1.0) <= dr.bar_lambda(n) * 3 / 1e-12


def test_refusals_and_the_band_rule():
    G = np.zeros((2, 6, 6))
    for thr in (0.0, 1.0, -1e-3, float("nan"), 1.5):
        assert oe.dopt_observability(G, [1, 2], thr) is None
    # threshold^2 >= 8 band(n): band = 128 eps up to n = 128, n eps above
    edge = np.sqrt(8 * 128 * dr.EPS)
    assert oe.dopt_observability(G, [1, 2], edge * (1 - 1e-9)) is None and oe.dopt_observability(G, [1, 2], edge * (1 + 1e-9)) is not None
    big = np.zeros((1, 300, 300))
    edge = np.sqrt(8 * 300 * dr.EPS)
    assert oe.dopt_observability(big, np.arange(300), edge * (1 - 1e-9)) is None
    assert oe.dopt_observability(big, np.arange(300), edge * (1 + 1e-9)) is not None


def test_an_eigenvalue_in_the_band_sets_bit_4_and_one_outside_does_not():
    n, thr = 6, 1e-2
    for off, want in ((0.5, 4), (-0.5, 4), (40.0, 0), (-40.0, 0)):  # in units of band lambda_max; the matrix is diagonal: exact
        M = np.diag([1.0, 0.5, 0.1, thr * thr + off * orf.band(n), 1e-7, 1e-9])
        got = oe.dopt_observability(M[None], np.arange(n), thr)
        assert got["status"][0] == want, (off, got["status"])
        assert got["n_observable"][0] == (4 if off > 0 else 3) and np.array_equal(np.sort(got["energy"][0]), [0, 0, 0] + [off < 0, 1, 1])


def test_a_nan_stays_in_its_candidate():
    G, cols, thr, _ = orf.case("obs24")
    G = np.concatenate([G, G[:2] * 3.0])
    clean = oe.dopt_observability(G, cols, thr)
    for bad in (np.nan, np.inf):
        H = G.copy()
        H[2, cols[5], cols[2]] = bad
        got = oe.dopt_observability(H, cols, thr)
        keep = [c for c in range(G.shape[0]) if c != 2]
        assert all(np.array_equal(got[k][keep], clean[k][keep]) for k in got)
        assert got["status"][2] == 1 and got["n_observable"][2] == 0
        assert all(np.all(np.isnan(got[k][2])) for k in ("energy", "margin", "eig", "vec"))


def test_power_of_two_scaling_changes_no_vector_bit():
    G, cols, thr, _ = orf.case("obs24")
    base = oe.dopt_observability(G, cols, thr)
    for p in (300, -300):
        got = oe.dopt_observability(G * 2.0 ** p, cols, thr)
        assert np.array_equal(got["eig"], base["eig"] * 2.0 ** p)
        assert all(np.array_equal(got[k], base[k]) for k in ("vec", "energy", "n_observable", "status", "margin"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the host pieces
# ---------------------------------------------------------------------------------------------------------------------------------
def test_observability_fields_and_merge(tmp_path):
    from flobaroid_amd import estimation as est
    from flobaroid_amd import excitation as exc

    result = {"n_observable_base_params": np.array([5, 3], dtype=np.int64), "unobservable_energy": np.zeros((2, 5)),
              "unobservable_params": [np.array([], dtype=np.int64), np.array([4, 17], dtype=np.int64)], "observability_threshold": 1e-6}
    f0, f1 = exc.observability_fields(result, 0), exc.observability_fields(result, 1)
    assert list(f1) == ["unobservable_params", "observability_threshold", "n_observable_base_params"]
    assert f1["unobservable_params"].dtype == np.int64 and f1["unobservable_params"].tolist() == [4, 17]
    assert f1["observability_threshold"] == 1e-6 and f1["n_observable_base_params"] == 3 and type(f1["n_observable_base_params"]) is int
    assert f0["unobservable_params"].dtype == np.int64 and f0["unobservable_params"].shape == (0,) and f0["n_observable_base_params"] == 5
    path = str(tmp_path / "trajectory.npz")
    np.savez(path, positions=np.zeros((3, 2)), **f1)
    data = np.load(path, allow_pickle=True)  # (as identifier.py reads it)
    assert data["unobservable_params"].dtype == np.int64 and int(data["n_observable_base_params"]) == 3
    assert float(data["observability_threshold"]) == 1e-6
    opt = {"dontChangeParams": [17, 2, 2]}
    assert est.merge_unobservable_params(opt, data) == [4] and opt["dontChangeParams"] == [17, 2, 4]
    assert est.merge_unobservable_params(opt, data) == [] and opt["dontChangeParams"] == [17, 2, 4]
    opt = {}
    assert est.merge_unobservable_params(opt, f1) == [4, 17] and opt == {"dontChangeParams": [4, 17]}
    opt = {"dontChangeParams": [9]}
    assert est.merge_unobservable_params(opt, f0) == [] and opt == {"dontChangeParams": [9]}  # (nothing unobservable: untouched)
    assert est.merge_unobservable_params(opt, {"positions": 1}) == [] and opt == {"dontChangeParams": [9]}


class _StandInEngine:
    """gram_grouped and dopt_observability of an Engine from NumPy and the emulation: the mapping of candidate_observability needs no GPU"""

    def __init__(self, Y):
        self.Y, self.calls = Y, []

    def gram_grouped(self, states, ncand, w=None):
        self.calls.append("gram_grouped")
        return np.einsum("crk,crj->ckj", self.Y, self.Y)

    def dopt_observability(self, G, cols, threshold=1e-6, prior=None, eigenvalues=False, vectors=False, device_out=None):
        self.calls.append("dopt_observability")
        return oe.dopt_observability(G, cols, threshold, prior=prior, eigenvalues=eigenvalues, vectors=vectors)


def test_candidate_observability_maps_as_pb_does():
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(3)
    P, rows = 12, 40
    Y = rng.standard_normal((2, rows, P))
    Y[1][:, 7] = 0.0  # candidate 1 does not excite columns 7 and 3
    Y[1][:, 3] = 0.0
    ic = np.array([9, 7, 0, 3, 11, 4])  # (in an order that is not sorted: Pb carries base parameter j to ic[j])
    eng = _StandInEngine(Y)
    r = exc.candidate_observability(eng, {}, 2, ic, {"observabilityThreshold": 1e-5})
    assert eng.calls == ["gram_grouped", "dopt_observability"]
    assert r["observability_threshold"] == 1e-5 and r["n_observable_base_params"].tolist() == [6, 4] and not r["ambiguous"].any()
    assert r["unobservable_params"][0].tolist() == [] and r["unobservable_params"][1].tolist() == [3, 7]
    assert r["unobservable_params"][1].dtype == np.int64 and r["unobservable_energy"].shape == (2, 6)
    for c in range(2):
        want = obr.observability(Y[c][:, ic], ic, P, 1e-5)
        f = exc.observability_fields(r, c)
        assert np.array_equal(f["unobservable_params"], want["unobservable_params"])
        assert f["n_observable_base_params"] == want["n_observable_base_params"] and f["observability_threshold"] == 1e-5
        assert np.abs(r["unobservable_energy"][c] - want["energy"]).max() <= 64 * dr.EPS
    assert exc.candidate_observability(eng, {}, 2, ic, {})["observability_threshold"] == 1e-6
    with pytest.raises(ValueError, match="host route"):
        exc.candidate_observability(eng, {}, 2, ic, {"useBasisProjection": 1})
    exc.candidate_observability(eng, {}, 2, ic, {"useBasisProjection": 0})
    # a prior: the analysis of the summed information -- candidate 1's two columns are excited by the prior
    prior = np.zeros((6, 6))
    prior[1, 1] = prior[3, 3] = 5.0
    assert exc.candidate_observability(eng, {}, 2, ic, {}, YtY_prior=prior)["n_observable_base_params"].tolist() == [6, 6]
