"""fbr_filtfilt / fbr_medfilt / fbr_central_diff and Data.preprocess(engine=...) on the device against the exact restatement
(tests/signal_reference.py, mpmath at 50 digits) at the edges of the kernels: every coefficient count, the reference's filter settings
at 0.2 .. 2 kHz, signals one sample longer than the padding, extended lengths of exactly one scan block and one sample more, 1 .. 130
columns (the chain kernel's second workgroup from 65 on), ld > ncols in host and device memory, a[0] != 1, every median window, records
shorter than the window, ties / signed zeros / infinities / denormals, the central difference where its five rules touch.

Cases, references and bars are those of tests/signal_cases.py; tests/test_signal_reference.py holds the g++ emulation of the kernels' text to
them on the CPU, with conditions (a) and (b) on every filtfilt case.  The filtfilt bar: max(10 x the emulation's deviation from the exact
result on the same input, 64 eps) x max|want| per channel.  Wide arrays: column c is base column c % 3 times a power of two and must
come back as that multiple bit for bit.

Zero phase: filtfilt(x[::-1]) == filtfilt(x)[::-1] does not hold in exact arithmetic (the transients of the padded ends differ between
the two sweep orders: 0.2 of the signal at the low cut-offs, 3e-5 at Wn = 0.3), so the device's asymmetry is held to the exact
asymmetry, to the two bars -- which is the property where it holds.  Scaled coefficients: [6 Hz, 5] at 2 kHz is left to condition (a)
(SciPy's own result moves by 1.4e-6 there), see tests/test_signal_reference.py.

Largest device / bar ratios seen on an MI355X (gfx950), every test green, no kernel change needed:
  a. filtfilt   0.18 (impulse at the block boundary, [3 Hz, 4] at 2 kHz); grid 0.13, scaled coefficients 0.10, reversed input 0.10 --
                0.10 is the emulation's own deviation: with and without FMA contraction the results differ by less than they err
  b. medfilt    equal as numbers on every case
  c. difference 0.20 of the derived bar (S = 5, 300 columns, varying steps)
  d. preprocess 0.62 of 10 x the host pipeline's deviation (Vdot at 2 kHz, median 5); Q and Tau <= 0.07, V <= 0.22"""
import functools

import numpy as np
import pytest

import signal_cases as sc
from common import load_topo

pytestmark = pytest.mark.gpu
EPS = sc.EPS


@functools.lru_cache(maxsize=None)
def _engine():
    from flobaroid_amd._lib import Engine

    return Engine(load_topo("threeLinks"))


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _report(group, case, ratio):
    print("RATIO %s %s %.3g" % (group, case, ratio))


def _on_device(fn, Z):
    """fn(tensor) on a device copy of Z; the tensor back as an array"""
    import torch

    Zd = torch.from_numpy(Z.copy()).cuda()
    fn(Zd)
    return Zd.cpu().numpy()


# ---- a. fbr_filtfilt ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", sc.GRID, ids=sc.grid_id)
def test_filtfilt_grid(g):
    """Every filter at every length, the column counts in turn: the base columns to the bar, the rest bit for bit their power-of-two
    multiples; ld = ncols + 3 in host and in device memory: the same bits, the extra columns untouched; the constant comes back."""
    fi, sk = g
    eng = _engine()
    r = sc.reference(fi, sk)
    b, a = sc.design(fi)
    ncols = sc.grid_ncols(g)
    nb = min(3, ncols)
    X = sc.wide(sc.base_channels(sc.length(fi, sk)), ncols)
    Y = eng.filtfilt(b, a, X.copy())
    dev = sc.deviations(Y[:, :nb], r)
    _report("a", sc.grid_id(g), (dev / r.bar[:nb]).max())
    assert np.all(dev <= r.bar[:nb]), dev / r.bar[:nb]
    sc.assert_scaled_columns(Y, ncols)
    Z = np.hstack([X, np.full((X.shape[0], 3), 7.25)])
    Zh = Z.copy()
    eng.filtfilt(b, a, Zh, ncols=ncols)
    assert np.array_equal(_bits(Zh[:, :ncols]), _bits(Y)) and np.all(Zh[:, ncols:] == 7.25)
    Zd = _on_device(lambda t: eng.filtfilt(b, a, t, ncols=ncols), Z)
    assert np.array_equal(_bits(Zd[:, :ncols]), _bits(Y)) and np.all(Zd[:, ncols:] == 7.25)
    if ncols >= 3:
        assert np.abs(Y[:, 1] - X[0, 1]).max() <= r.bar[1] + sc.dc_gain_error(fi) * X[0, 1] * (1 + 4 * EPS)


@pytest.mark.parametrize("fi", [fi for fi in range(len(sc.FILTERS)) if fi not in sc.SCALED_EXCLUDED], ids=lambda fi: sc.FILTER_IDS[fi])
def test_filtfilt_scaled_coefficients(fi):
    """(3.7 b, 3.7 a) gives the exact result of (b, a) to the bar"""
    b, a = sc.design(fi)
    r = sc.reference_scaled(fi, 2)
    Y = _engine().filtfilt(3.7 * b, 3.7 * a, np.array(sc.base_channels(sc.length(fi, 2))))
    dev = sc.deviations(Y, r)
    _report("a", "scaled-" + sc.FILTER_IDS[fi], (dev / r.bar).max())
    assert np.all(dev <= r.bar), dev / r.bar


@pytest.mark.parametrize("fi", range(len(sc.FILTERS)), ids=sc.FILTER_IDS)
def test_filtfilt_reversed_input(fi):
    """the reversed signal to its own bar, and the asymmetry between the two runs equal to the exact one to the two bars"""
    b, a = sc.design(fi)
    r, rr = sc.reference(fi, 2), sc.reference_reversed(fi, 2)
    X = np.array(sc.base_channels(sc.length(fi, 2)))
    Y = _engine().filtfilt(b, a, X.copy())
    Yr = _engine().filtfilt(b, a, np.ascontiguousarray(X[::-1]))
    dev = sc.deviations(Yr, rr)
    asym = sc.asymmetry_deviation(Y, Yr, r, rr)
    _report("a", "reversed-" + sc.FILTER_IDS[fi], max((dev / rr.bar).max(), (asym / (r.bar + rr.bar)).max()))
    assert np.all(dev <= rr.bar), dev / rr.bar
    assert np.all(asym <= r.bar + rr.bar), asym / (r.bar + rr.bar)


@pytest.mark.parametrize("fi", range(len(sc.FILTERS)), ids=sc.FILTER_IDS)
def test_filtfilt_impulse_at_the_block_boundary(fi):
    """a unit impulse at the last sample of the first scan block, at the first of the second, at both"""
    b, a = sc.design(fi)
    r = sc.reference_impulse(fi)
    Y = _engine().filtfilt(b, a, sc.impulse_channels(fi))
    dev = sc.deviations(Y, r)
    _report("a", "impulse-" + sc.FILTER_IDS[fi], (dev / r.bar).max())
    assert np.all(dev <= r.bar), dev / r.bar


@pytest.mark.parametrize("fi", range(len(sc.FILTERS)), ids=sc.FILTER_IDS)
def test_filtfilt_nan_stays_in_its_channel(fi):
    """65 columns, a NaN in column 1: every other column keeps the bits of the run without it (host and device memory)"""
    eng = _engine()
    b, a = sc.design(fi)
    X = sc.wide(sc.base_channels(sc.length(fi, 2)), 65)
    Y = eng.filtfilt(b, a, X.copy())
    Xn = X.copy()
    Xn[X.shape[0] // 2, 1] = np.nan
    keep = np.arange(65) != 1
    for got in (eng.filtfilt(b, a, Xn.copy()), _on_device(lambda t: eng.filtfilt(b, a, t), Xn)):
        assert np.array_equal(_bits(got[:, keep]), _bits(Y[:, keep])) and np.isnan(got[:, 1]).any()


# ---- b. fbr_medfilt -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sc.MED_K)
def test_medfilt_is_the_exact_median(k):
    """records shorter than, as long as and longer than the window; all-tie columns, signed zeros, infinities, denormals, ramps; as numbers"""
    eng = _engine()
    for S in sc.med_lengths(k):
        for ncols in sc.MED_NCOLS:
            want = sc.med_reference(k, S, ncols)
            Z = np.hstack([sc.med_input(S, ncols), np.full((S, 2), -3.5)])
            got = [eng.medfilt(k, Z.copy(), ncols=ncols)]
            if S == 257:
                got.append(_on_device(lambda t: eng.medfilt(k, t, ncols=ncols), Z))
            for G in got:
                assert np.all(G[:, :ncols] == want) and np.all(G[:, ncols:] == -3.5), (S, ncols)


def test_medfilt_and_central_diff_refusals():
    from flobaroid_amd._lib import FbrError

    eng = _engine()
    for k in (0, 2, 32, 33):
        with pytest.raises(FbrError):
            eng.medfilt(k, np.zeros((40, 2)))
    with pytest.raises(FbrError):
        eng.central_diff(np.zeros((4, 2)), np.arange(4.0))


# ---- c. fbr_central_diff --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,ncols,steps", sc.CD_CASES, ids=str)
def test_central_diff_within_the_derived_bar(S, ncols, steps):
    A, T = sc.cd_input(S, ncols, steps)
    ratio = sc.cd_ratio(_engine().central_diff(A.copy(), T.copy()), S, ncols, steps)
    _report("c", "%d-%d-%s" % (S, ncols, steps), ratio)
    assert ratio <= 1.0


# ---- d. Data.preprocess ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fs,k", sc.PRE_CASES, ids=str)
def test_preprocess_against_the_exact_chain(Fs, k):
    """Q, V, Vdot, Tau of the device pipeline: at most 10 x the host SciPy pipeline's deviation from the exact chain (floor 64 eps max|want|)"""
    exact, bars = sc.pre_reference(Fs, k)
    ratios = {name: sc.pre_deviation(got, exact[name]) / bars[name] for name, got in zip(sc.PRE_NAMES, sc.pre_run(Fs, k, _engine()))}
    for name in sc.PRE_NAMES:
        _report("d", "%g-%d-%s" % (Fs, k, name), ratios[name])
    assert max(ratios.values()) <= 1.0, ratios
