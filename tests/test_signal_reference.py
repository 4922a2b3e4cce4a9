"""The signal conditioning off the GPU.  (1) The exact restatement tests/signal_reference.py (mpmath, 50 digits) is pinned on SciPy, on
Data._central_diff and on the reference's own Data.preprocess outputs.  (2) The HIP-free text of csrc/fbr_signal.h under g++
(tests/emul/signal_emul.cpp: the design step, passes A / B / C block by block, the median, the central difference) is held to the exact
restatement on every case of tests/test_gpu_signal_edges.py, which settles the cases and the bars before a GPU is asked: conditions (a)
and (b) of tests/signal_cases.py on every filtfilt case, the power-of-two identity of the wide arrays, the leading dimension, a NaN
channel, scaled coefficients, impulses at the block boundary, the medians as numbers, the central difference to its derived bar, and
Data.preprocess with the emulation as its engine against the exact chain."""
import json
import os

import numpy as np
import pytest

import signal_cases as sc
import signal_reference as sr
from common import GOLDEN

EPS = sc.EPS
EMU = sc.EmulEngine()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


# ---- (1) the exact restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", range(1, 12))
def test_reference_filtfilt_is_scipys_on_well_conditioned_filters(order):
    """orders 1 .. 11 at Wn = 0.3 (cond <= 1.7e3): scipy.signal.filtfilt == the exact restatement to 64 eps cond"""
    import scipy.signal as sig

    b, a = sig.butter(order, 0.3)
    cond = float(np.abs(a).sum() / abs(a.sum()))
    assert cond <= 1.7e3
    rng = np.random.default_rng(order)
    S = 3 * (order + 1) + 1 + 40 * order
    x = np.cumsum(rng.standard_normal(S)) * 0.1 + 3.0
    want = sr.filtfilt(b, a, x)
    assert sr.deviation(sig.filtfilt(b, a, x), want) <= 64 * EPS * cond * max(abs(float(w)) for w in want)
    with pytest.raises(ValueError):
        sr.filtfilt(b, a, x[:3 * (order + 1)])


def test_reference_filtfilt_normalises_and_pads_like_scipy():
    """a[0] != 1 and coefficient vectors of different lengths"""
    import scipy.signal as sig

    rng = np.random.default_rng(5)
    x = rng.standard_normal(60)
    for b, a in (([0.3, 0.2], [2.0, -0.8, 0.3]), ([0.5, 0.1, 0.2, 0.05], [-1.5, 0.4])):
        want = sr.filtfilt(b, a, x)
        assert sr.deviation(sig.filtfilt(b, a, x), want) <= 1e-13 * max(abs(float(w)) for w in want)


def test_reference_lfilter_zi_is_scipys():
    import scipy.signal as sig

    b, a = sig.butter(6, 0.3)
    got = [float(v) for v in sr.lfilter_zi(sr._exact(b), sr._exact(a))]
    assert np.abs(np.array(got) - sig.lfilter_zi(b, a)).max() <= 1e-12


@pytest.mark.parametrize("k", [1, 3, 7, 31])
def test_reference_medfilt_is_scipys(k):
    import scipy.signal as sig

    for S in (1, 2, k - 1 or 1, k, 90):
        X = sc.med_input(S, 5)
        for c in range(5):
            got = np.array(sr.medfilt(k, X[:, c].tolist()))
            assert np.all(got == sig.medfilt(X[:, c], k)), (S, c)


@pytest.mark.parametrize("S,ncols,steps", [c for c in sc.CD_CASES if c[1] == 1 or c[0] == 257], ids=str)
def test_reference_central_diff_is_the_host_version(S, ncols, steps):
    from flobaroid_amd.data import Data

    A, T = sc.cd_input(S, ncols, steps)
    assert sc.cd_ratio(Data._central_diff(A, T), S, ncols, steps) <= 1.0
    with pytest.raises(ValueError):
        sr.central_diff(A[:4, 0], T[:4])


def test_reference_preprocess_reproduces_the_reference_outputs():
    """the exact chain on the fixture of the reference's own Data.preprocess: Q, V, Vdot, Tau to the fixture's 1e-9"""
    import scipy.signal as sig

    z = np.load(os.path.join(GOLDEN, "ref_host_functions.npz"), allow_pickle=True)
    opt = json.loads(str(z["pre_opt"]))
    Fs = float(z["pre_Fs"])
    lp = [sig.butter(order, fc / (Fs / 2), btype="low", analog=False) for fc, order in (opt["filterLowPass1"], opt["filterLowPass2"])]
    assert opt["useDeg"] == 0
    for j in range(opt["num_dofs"]):
        out = sr.preprocess(z["pre_Q"][:, j], z["pre_Tau"][:, j], z["pre_T"], opt["filterMedianSize"], lp[0], lp[1])
        for name, got in zip(sc.PRE_NAMES, out):
            want = z["pre_out_" + name]
            assert sr.deviation(want[:, j], got) <= 1e-9 * max(1.0, np.abs(want).max()), (name, j)


# ---- (2) the emulation against the exact restatement: filtfilt ------------------------------------------------------------------------------
def test_emulation_runs_the_headers_block_length():
    assert sc.emul().sig_block_length() == sc.LB


def test_emulation_refusals():
    b, a = sc.design(3)
    with pytest.raises(sc.EmulError):
        EMU.filtfilt(b, a, np.zeros((18, 2)))
    with pytest.raises(sc.EmulError):
        EMU.filtfilt(np.r_[b, np.zeros(7)], np.r_[a, np.zeros(7)], np.zeros((100, 2)))  # 13 coefficients
    for k in (0, 2, 32, 33):
        with pytest.raises(sc.EmulError):
            EMU.medfilt(k, np.zeros((40, 2)))
    with pytest.raises(sc.EmulError):
        EMU.central_diff(np.zeros((4, 2)), np.arange(4.0))


@pytest.mark.parametrize("g", sc.GRID, ids=sc.grid_id)
def test_emulation_filtfilt_grid(g):
    """Conditions (a) and (b) on every grid case; the wide array: columns bit for bit power-of-two multiples of the base columns, the same
    bits with ld = ncols + 3, the three extra columns untouched."""
    fi, sk = g
    r = sc.reference(fi, sk)
    sc.check_conditions(r)
    b, a = sc.design(fi)
    ncols = sc.grid_ncols(g)
    X = sc.wide(sc.base_channels(sc.length(fi, sk)), ncols)
    Y = EMU.filtfilt(b, a, X.copy())
    assert np.array_equal(_bits(Y[:, :min(3, ncols)]), _bits(r.emul[:, :min(3, ncols)]))
    sc.assert_scaled_columns(Y, ncols)
    Z = np.hstack([X, np.full((X.shape[0], 3), 7.25)])
    EMU.filtfilt(b, a, Z, ncols=ncols)
    assert np.array_equal(_bits(Z[:, :ncols]), _bits(Y)) and np.all(Z[:, ncols:] == 7.25)
    # the constant comes back: to the bar, beyond what the coefficients' own DC gain moves it by
    if ncols >= 3:
        assert np.abs(Y[:, 1] - X[0, 1]).max() <= r.bar[1] + sc.dc_gain_error(fi) * X[0, 1] * (1 + 4 * EPS)


@pytest.mark.parametrize("fi", range(len(sc.FILTERS)), ids=sc.FILTER_IDS)
def test_emulation_filtfilt_properties(fi):
    """At the length with a second block of one sample: scaled coefficients, the reversed input (conditions (a), (b) on both), impulses
    either side of the block boundary, a NaN channel."""
    sk = 2
    b, a = sc.design(fi)
    r = sc.reference(fi, sk)
    if fi not in sc.SCALED_EXCLUDED:
        sc.check_conditions(sc.reference_scaled(fi, sk))
    rr = sc.reference_reversed(fi, sk)
    sc.check_conditions(rr)
    asym = sc.asymmetry_deviation(r.emul, rr.emul, r, rr)
    assert np.all(asym <= r.bar + rr.bar), asym / (r.bar + rr.bar)
    sc.check_conditions(sc.reference_impulse(fi))
    X = sc.wide(sc.base_channels(sc.length(fi, sk)), 65)
    Y = EMU.filtfilt(b, a, X.copy())
    Xn = X.copy()
    Xn[X.shape[0] // 2, 1] = np.nan
    EMU.filtfilt(b, a, Xn)
    keep = np.arange(65) != 1
    assert np.array_equal(_bits(Xn[:, keep]), _bits(Y[:, keep])) and np.isnan(Xn[:, 1]).any()


def test_scaled_coefficients_case_that_scipy_cannot_do():
    """[6 Hz, 5] at 2 kHz (cond 1.3e10): rounding (3.7 b, 3.7 a) moves SciPy's own result by more than 1e-6 of the signal -- by condition
    (a) that is not a case of the scaled-coefficients check; every other filter is."""
    assert [sc.FILTERS[fi][0] for fi in sc.SCALED_EXCLUDED] == ["lp6Hz5@2000"]
    r = sc.reference_scaled(sc.SCALED_EXCLUDED[0], 2)
    assert np.any(r.dev_scipy > 1e-6 * r.scale)


# ---- medfilt, central difference, the chain --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sc.MED_K)
def test_emulation_medfilt_is_the_exact_median(k):
    for S in sc.med_lengths(k):
        for ncols in sc.MED_NCOLS:
            X = sc.med_input(S, ncols)
            Z = np.hstack([X, np.full((S, 2), -3.5)])
            EMU.medfilt(k, Z, ncols=ncols)
            assert np.all(Z[:, :ncols] == sc.med_reference(k, S, ncols)) and np.all(Z[:, ncols:] == -3.5), (S, ncols)


@pytest.mark.parametrize("S,ncols,steps", sc.CD_CASES, ids=str)
def test_emulation_central_diff_within_the_derived_bar(S, ncols, steps):
    A, T = sc.cd_input(S, ncols, steps)
    assert sc.cd_ratio(EMU.central_diff(A.copy(), T.copy()), S, ncols, steps) <= 1.0


@pytest.mark.parametrize("Fs,k", sc.PRE_CASES, ids=str)
def test_emulation_preprocess_against_the_exact_chain(Fs, k):
    exact, bars = sc.pre_reference(Fs, k)
    for name, got in zip(sc.PRE_NAMES, sc.pre_run(Fs, k, EMU)):
        assert sc.pre_deviation(got, exact[name]) <= bars[name], name
