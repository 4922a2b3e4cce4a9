"""The D-optimality arithmetic off the GPU: the 50-digit reference (tests/dopt_reference.py) is pinned on closed forms, LAPACK's own error
against it is measured (the number the bars are built from), the HIP-free text of csrc/fbr_dopt.h (g++, tests/emul/dopt_emul.cpp) is held
to the bars on every matrix family, and a program of its own runs that text under the address and undefined-behaviour sanitizers.

Measured here (g++, -ffp-contract=off), worst error / bar over the families: eigenvalues 0.07, neg_log_det 0.003, Cmat 0.44."""
import os
import subprocess

import numpy as np
import pytest

import dopt_emul_lib as de
import dopt_reference as dr

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_reference_on_closed_forms():
    r = dr.mp_reference(np.array([[3.0]]), 1e-4, 2.0)
    assert r["ev"][0] == 3.0 and r["lambda_max"] == 3.0 and r["delta"] == 1e-4 * 3.0 and r["n_observable"] == 1
    assert abs(r["neg_log_det"] + np.log(3.0 * (1 + 1e-4))) <= 2 * dr.EPS and abs(r["Cmat"][0, 0] + 4.0 / (3.0 * (1 + 1e-4))) <= 2 * dr.EPS
    a, b, c = 2.0, 0.75, 5.0  # [[a, b], [b, c]]: (a + c) / 2 -+ sqrt(((a - c) / 2)^2 + b^2)
    r = dr.mp_reference(np.array([[a, b], [b, c]]), 1e-3)
    h = np.sqrt(np.longdouble((a - c) / 2) ** 2 + np.longdouble(b) ** 2)
    want = np.array([float((a + c) / 2 - h), float((a + c) / 2 + h)])
    assert np.abs(r["ev"] - want).max() <= 2 * dr.EPS * want[1]
    dl = 1e-3 * want[1]
    det = (a + dl) * (c + dl) - b * b
    assert np.abs(r["Cmat"] - (-2.0 / det) * np.array([[c + dl, -b], [-b, a + dl]])).max() <= 8 * dr.EPS * np.abs(r["Cmat"]).max()
    d = np.array([4.0, 1.0, 1.0, 1e-7, 0.0])
    r = dr.mp_reference(np.diag(d), 1e-4)
    assert np.array_equal(r["ev"], np.sort(d)) and r["n_observable"] == 3 and r["delta"] == 1e-4 * 4.0
    assert abs(r["neg_log_det"] + np.sum(np.log(d + 1e-4 * 4.0))) <= 64 * dr.EPS
    assert np.abs(np.diag(r["Cmat"]) + 2.0 / (d + 1e-4 * 4.0)).max() <= 4 * dr.EPS * 2.0 / 4e-4 and r["Cmat"][0, 1] == 0.0


def test_lapack_error_is_what_the_bars_are_built_from():
    """eigvalsh against the reference over every family: at most LAPACK_WORST of its size class (6.4e-16 up to n = 8, 1.1e-15 up to 32,
    1.2e-15 up to 65; the two larger ones are set by the oracle Grams of threeLinks and KUKA, 1.08e-15 and 1.13e-15, which
    test_emulation_on_oracle_grams prints), and within a factor of 4 of it -- the bars are 16 x these numbers, floored at n eps"""
    worst = {k: 0.0 for k in dr.LAPACK_WORST}
    for name in dr.CASES:
        n = len(dr.case(name)[1])
        k = min(k for k in dr.LAPACK_WORST if n <= k)
        worst[k] = max(worst[k], max(r["lapack_err"] for r in dr.reference(name)))
    print("LAPACK worst error / lambda_max by size class:", worst)
    for k, v in worst.items():
        assert dr.LAPACK_WORST[k] / 4 <= v <= dr.LAPACK_WORST[k], (k, v)
    assert dr.bar_lambda(5) == 16 * 6.4e-16 and dr.bar_lambda(64) == 16 * 1.2e-15 and dr.bar_lambda(213) == 213 * dr.EPS


@pytest.mark.parametrize("name", dr.CASES)
def test_emulation_within_the_bars(name):
    G, cols, reg, prior, scale = dr.case(name)
    got = de.dopt_terms(G, cols, reg, prior, scale, nt=64)
    w = dr.check_against_reference(name, got, "emulation")
    print(name, "worst error / bar:", w)
    # the number of lanes, and leaving eig / Cmat out, change no bit
    for nt, kw in ((256, {}), (1, {}), (64, {"eigenvalues": False, "weights": False})):
        again = de.dopt_terms(G, cols, reg, prior, scale, nt=nt, **kw)
        assert all(np.array_equal(again[k], got[k], equal_nan=True) for k in again), (name, nt)


@pytest.mark.parametrize("case", [c for c in dr.ROBOTS if c[4] != 70], ids=lambda c: f"{c[0]}-{c[3]}x{c[4]}")
def test_emulation_on_oracle_grams(case):
    """(WALK-MAN with 70 samples is left to the device: the serial emulation of n = 213 takes seconds per factorisation)"""
    G, cols = dr.oracle_grams(*case)
    scale = np.linspace(0.5, 1.5, case[3])
    dr.check_robot(case, de.dopt_terms(G, cols, 1e-4, None, scale, nt=256), scale, where="emulation")


def test_emulation_zero_matrix_and_singular_factorisation():
    G, cols, reg, _, _ = dr.case("zero")
    got = de.dopt_terms(G, cols, reg)
    assert np.all(got["eig"] == 0.0) and np.all(got["delta"] == reg * 1e-30) and np.all(got["n_observable"] == 0)
    assert np.all(np.isfinite(got["Cmat"])) and np.all(got["status"] == 0)
    Y = np.random.default_rng(3).standard_normal((3, 5))
    Ms = [Y.T @ Y, np.eye(5), np.diag([1.0, 1.0, 0.0, 1.0, 1.0])]
    G, cols = dr.embed(Ms, None, np.random.default_rng(4))
    got = de.dopt_terms(G, cols, 0.0)
    assert got["status"][1] == 0 and got["status"][2] == 2 and np.all(np.isnan(got["Cmat"][2])) and np.all(np.isfinite(got["Cmat"][1]))
    assert got["status"][0] in (0, 2)  # (rank 3 of 5 in floating point: the last pivots are roundings of either sign)
    assert np.all(np.isfinite(got["neg_log_det"][1:])) and got["lambda_max"][2] == 1.0


def test_emulation_scaling_is_exact_and_a_nan_stays_in_its_candidate():
    G, cols, reg, prior, scale = dr.case("logspace24")
    G = G * 2.0 ** 210  # (lambda_max 2^-300 G stays above the floor 1e-30 of delta)
    base = de.dopt_terms(G, cols, reg)
    for p in (300, -300):
        got = de.dopt_terms(G * 2.0 ** p, cols, reg)
        for k in ("eig", "lambda_max", "delta"):
            assert np.array_equal(got[k], base[k] * 2.0 ** p), (p, k)
        assert np.array_equal(got["Cmat"], base["Cmat"] * 2.0 ** -p) and np.array_equal(got["n_observable"], base["n_observable"])
    Gn = np.concatenate([G, G[:2]])
    clean = de.dopt_terms(Gn, cols, reg)
    Gn[2, cols[3], cols[1]] = np.nan
    got = de.dopt_terms(Gn, cols, reg)
    for c in (0, 1, 3, 4):
        assert all(np.array_equal(got[k][c], clean[k][c]) for k in got), c
    assert got["status"][2] == 1 and got["n_observable"][2] == 0 and np.all(np.isnan(got["eig"][2])) and np.all(np.isnan(got["Cmat"][2]))
    assert all(np.isnan(got[k][2]) for k in ("neg_log_det", "lambda_max", "delta"))
    Gn[2, cols[3], cols[1]] = np.inf
    assert de.dopt_terms(Gn, cols, reg)["status"].tolist() == [0, 0, 1, 0, 0]
    # an entry above the diagonal of M is not read at all
    Gn[2, cols[3], cols[1]] = G[2, cols[3], cols[1]]
    Gn[2, cols[1], cols[3]] = np.nan
    assert de.dopt_terms(Gn, cols, reg)["status"].tolist() == [0, 0, 0, 0, 0]


def test_halvings_are_fixed_by_n():
    h = de.emul().dopt_emul_halvings
    assert [h(n) for n in (1, 2, 3, 64, 65, 213, 512)] == [56, 57, 58, 62, 63, 64, 65]


def test_arithmetic_under_the_sanitizers(tmp_path):
    """tests/emul/dopt_sanitize.cpp, a program of its own, built with -fsanitize=address,undefined and run here on the CPU"""
    exe = str(tmp_path / "dopt_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(_HERE, "emul", "dopt_sanitize.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), (run.stdout[-2000:], run.stderr[-4000:])
