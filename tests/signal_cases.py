"""Cases, exact references and bars of the signal-conditioning edge tests, shared by the CPU side (tests/test_signal_reference.py: the g++
emulation tests/emul/signal_emul.cpp of csrc/fbr_signal.h against tests/signal_reference.py) and the GPU side
(tests/test_gpu_signal_edges.py).  Every reference is built once per process (functools.lru_cache) and never changed.

The rounding bar of a filtfilt case: per channel max(10 r, 64 eps) * max|want|, r the largest deviation of the emulation from the exact
reference over the channels of the case, each relative to its channel's max|want| (so a channel on which the emulation happens to
round luckily does not get a bar of its own), under two conditions asserted on the CPU: (a) SciPy's own error <= 1e-6 relative, (b) the
emulation's deviation <= 4 x SciPy's, with the same floor."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import signal_reference as sr
from common import ROOT

EPS = float(np.finfo(np.float64).eps)
_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "signal_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libsignal_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_dp = ctypes.POINTER(ctypes.c_double)
_lib = None


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC] + [os.path.join(_CSRC, h) for h in ("fbr_signal.h", "fbr_math.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


class EmulError(ValueError):
    pass


class EmulEngine:
    """The three entry points with the signatures of flobaroid_amd._lib.Engine, on NumPy arrays, run by the emulation."""

    @staticmethod
    def _arr(X):
        if not (isinstance(X, np.ndarray) and X.ndim == 2 and X.flags.c_contiguous and X.dtype == np.float64):
            raise ValueError("expected a C-contiguous 2-D float64 ndarray")
        return X.ctypes.data_as(_dp), ctypes.c_long(X.shape[0]), int(X.shape[1])

    def filtfilt(self, b, a, X, ncols=None):
        b, a = np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(a, dtype=np.float64)
        if b.size != a.size:
            n = max(b.size, a.size)
            b, a = np.r_[b, np.zeros(n - b.size)], np.r_[a, np.zeros(n - a.size)]
        p, S, ld = self._arr(X)
        if emul().sig_filtfilt(b.ctypes.data_as(_dp), a.ctypes.data_as(_dp), int(b.size), p, S, ld if ncols is None else int(ncols), ld):
            raise EmulError("fbr_filtfilt")
        return X

    def medfilt(self, k, X, ncols=None):
        p, S, ld = self._arr(X)
        if emul().sig_medfilt(int(k), p, S, ld if ncols is None else int(ncols), ld):
            raise EmulError("fbr_medfilt")
        return X

    def central_diff(self, A, times):
        p, S, ld = self._arr(A)
        T = np.ascontiguousarray(times, dtype=np.float64)
        assert T.shape == (A.shape[0],)
        D = np.zeros_like(A)
        if emul().sig_central_diff(p, T.ctypes.data_as(_dp), D.ctypes.data_as(_dp), S, ld):
            raise EmulError("fbr_central_diff")
        return D


LB = 2048  # FBR_SIG_LB (asserted against the header in tests/test_signal_reference.py)

# ---- filtfilt -----------------------------------------------------------------------------------------------------------------------------
# the reference's three low-pass settings at three sampling rates, then every coefficient count at Wn = 0.3
FILTERS = [("lp%dHz%d@%d" % (fc, order, fs), order, fc / (fs / 2.0)) for fs in (200, 1000, 2000) for fc, order in ((8, 5), (6, 5), (3, 4))]
FILTERS += [("nc%d" % nc, nc - 1, 0.3) for nc in range(2, 13)]
FILTER_IDS = [f[0] for f in FILTERS]
S_KINDS = ("pad+1", "Le=LB", "Le=LB+1", "2LB+77")
NCOLS = (1, 3, 64, 65, 130)
GRID = [(fi, sk) for fi in range(len(FILTERS)) for sk in range(len(S_KINDS))]


def grid_id(g):
    return "%s-%s-n%d" % (FILTERS[g[0]][0], S_KINDS[g[1]], grid_ncols(g))


def grid_ncols(g):
    return NCOLS[(g[0] * len(S_KINDS) + g[1]) % len(NCOLS)]


@functools.lru_cache(maxsize=None)
def design(fi):
    import scipy.signal as sig

    _, order, wn = FILTERS[fi]
    b, a = sig.butter(order, wn)
    return np.ascontiguousarray(b), np.ascontiguousarray(a)


def cond(fi):
    a = design(fi)[1]
    return float(np.abs(a).sum() / abs(a.sum()))


def length(fi, sk):
    nc = FILTERS[fi][1] + 1
    pad = 3 * nc
    return (pad + 1, LB - 2 * pad, LB + 1 - 2 * pad, 2 * LB + 77)[sk]


@functools.lru_cache(maxsize=None)
def base_channels(S):
    """(S, 3): a random walk, a constant, 1e6 + a unit-scale walk"""
    rng = np.random.default_rng(S)
    X = np.empty((S, 3))
    X[:, 0] = np.cumsum(rng.standard_normal(S)) * 0.1 + 3.0 * rng.standard_normal()
    X[:, 1] = 2.7182818284590451
    X[:, 2] = 1e6 + np.cumsum(rng.standard_normal(S)) * 0.05
    X.setflags(write=False)
    return X


def impulse_channels(fi):
    """(S, 3), S = LB + 77: a unit impulse at extended sample LB - 1 (the last of the first block), at LB (the first of the second), both"""
    pad = 3 * (FILTERS[fi][1] + 1)
    X = np.zeros((LB + 77, 3))
    X[LB - 1 - pad, 0] = X[LB - pad, 1] = 1.0
    X[LB - 1 - pad, 2] = X[LB - pad, 2] = 1.0
    return X


def exponents(ncols):
    """power-of-two exponent of column c (0 for the three base columns, then -20 .. 20)"""
    e = (np.arange(ncols) * 7 + 3) % 41 - 20
    e[:3] = 0
    return e


def wide(base, ncols):
    """(S, ncols): column c = base channel c % 3 times 2^e_c, exactly"""
    return np.ascontiguousarray(np.ldexp(base[:, np.arange(ncols) % 3], exponents(ncols)[None, :]))


def assert_scaled_columns(Y, ncols, what=""):
    """column c of Y is column c % 3 times 2^e_c bit for bit (linearity: scaling by a power of two commutes with every rounding)"""
    want = np.ldexp(Y[:, np.arange(ncols) % 3], exponents(ncols)[None, :])
    assert np.array_equal(Y[:, :ncols].view(np.int64), want.view(np.int64)), what


class Ref:
    """exact outputs (list of channels of mpf), their float64 roundings, the deviations of SciPy and of the emulation, the bars"""


def _reference(b, a, X, b_run=None, a_run=None):
    """Exact reference of filtfilt(b, a) on the channels of X; SciPy and the emulation run with (b_run, a_run) (default: the same pair)."""
    import scipy.signal as sig

    b_run, a_run = (b, a) if b_run is None else (b_run, a_run)
    r = Ref()
    nch = X.shape[1]
    r.exact = [sr.filtfilt(b, a, X[:, c]) for c in range(nch)]
    r.want = np.array([sr.to_float(w) for w in r.exact]).T
    r.scale = np.abs(r.want).max(axis=0)
    sp = sig.filtfilt(b_run, a_run, X, axis=0)
    em = EmulEngine().filtfilt(b_run, a_run, X.copy())
    r.emul = em
    r.dev_scipy = np.array([sr.deviation(sp[:, c], r.exact[c]) for c in range(nch)])
    r.dev_emul = np.array([sr.deviation(em[:, c], r.exact[c]) for c in range(nch)])
    r.rel = float((r.dev_emul / r.scale).max())
    r.bar = np.maximum(10 * r.rel, 64 * EPS) * r.scale
    return r


def check_conditions(r):
    """(a) SciPy's own error <= 1e-6 relative: the (b, a) form is meaningful; (b) the emulation's deviation <= 4 x SciPy's (floor 64 eps)"""
    assert np.all(r.dev_scipy <= 1e-6 * r.scale), (r.dev_scipy / r.scale)
    lim = np.maximum(4 * (r.dev_scipy / r.scale).max(), 64 * EPS) * r.scale
    assert np.all(r.dev_emul <= lim), (r.dev_emul / r.scale, r.dev_scipy / r.scale)


def deviations(got, r):
    """per channel max |got - exact| of the (up to three) base channels of got"""
    return np.array([sr.deviation(got[:, c], r.exact[c]) for c in range(min(got.shape[1], len(r.exact)))])


@functools.lru_cache(maxsize=None)
def reference(fi, sk):
    """reference of grid case (filter fi, length kind sk) on the walk channels (the first min(3, ncols) of them are used)"""
    b, a = design(fi)
    return _reference(b, a, base_channels(length(fi, sk)))


@functools.lru_cache(maxsize=None)
def reference_reversed(fi, sk):
    b, a = design(fi)
    return _reference(b, a, np.ascontiguousarray(base_channels(length(fi, sk))[::-1]))


@functools.lru_cache(maxsize=None)
def reference_scaled(fi, sk):
    """exact: the unscaled pair; SciPy and the emulation: (3.7 b, 3.7 a)"""
    b, a = design(fi)
    return _reference(b, a, base_channels(length(fi, sk)), 3.7 * b, 3.7 * a)


@functools.lru_cache(maxsize=None)
def reference_impulse(fi):
    b, a = design(fi)
    return _reference(b, a, impulse_channels(fi))


# [6 Hz, 5] at 2 kHz: rounding the scaled pair moves SciPy's own result by 1.4e-6 of the signal, beyond condition (a)
SCALED_EXCLUDED = [FILTER_IDS.index("lp6Hz5@2000")]


def asymmetry_deviation(got, got_rev, r, rr):
    """Per channel max |(got_rev reversed - got) - (the same difference of the exact results)|.  filtfilt(x[::-1]) is filtfilt(x)[::-1] only
    up to the transients of the padded ends (a forward-backward against a backward-forward sweep: 0.2 of the signal at the low
    cut-offs, 3e-5 at Wn = 0.3, in exact arithmetic), so the device's asymmetry is held to the exact one, to the two bars."""
    out = []
    for c in range(len(r.exact)):
        e, er = r.exact[c], rr.exact[c][::-1]
        out.append(float(max(abs((sr.mpf(float(got_rev[-1 - t, c])) - sr.mpf(float(got[t, c]))) - (er[t] - e[t])) for t in range(len(e)))))
    return np.array(out)


def dc_gain_error(fi):
    """|(sum b / sum a)^2 - 1| of the float64 coefficients, exactly: what the two sweeps move a constant by in exact arithmetic"""
    b, a = design(fi)
    return float(abs((sum(sr._exact(b)) / sum(sr._exact(a))) ** 2 - 1))


# ---- medfilt ------------------------------------------------------------------------------------------------------------------------------
MED_K = list(range(1, 32, 2))
MED_NCOLS = (1, 3, 257)


def med_lengths(k):
    return sorted({S for S in (1, 2, k // 2, k - 1, k, 257) if S >= 1})


@functools.lru_cache(maxsize=None)
def med_input(S, ncols):
    """column c: type c % 5 -- integers of -2 .. 2 (all ties), signed zeros among +-1, +-inf among normals, denormals, a strictly monotone
    ramp (rising or falling)"""
    rng = np.random.default_rng(1000 * S + ncols)
    X = np.empty((S, ncols))
    for c in range(ncols):
        t = c % 5
        if t == 0:
            X[:, c] = rng.integers(-2, 3, S)
        elif t == 1:
            X[:, c] = rng.choice([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], S)
        elif t == 2:
            X[:, c] = rng.choice([np.inf, -np.inf, 1.5, -2.5, 0.0, 1e300], S)
        elif t == 3:
            X[:, c] = rng.integers(-3, 4, S) * 5e-324
        else:
            X[:, c] = (np.arange(S) * 0.37 - 11.0) * (-1.0 if c % 2 else 1.0)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def med_reference(k, S, ncols):
    X = med_input(S, ncols)
    W = np.array([sr.medfilt(k, X[:, c].tolist()) for c in range(ncols)]).T.reshape(S, ncols)
    W.setflags(write=False)
    return W


# ---- central difference ---------------------------------------------------------------------------------------------------------------------
CD_CASES = [(S, ncols, steps) for S in (5, 6, 7, 257) for ncols in (1, 300) for steps in ("uniform", "varying")]


@functools.lru_cache(maxsize=None)
def cd_input(S, ncols, steps):
    rng = np.random.default_rng(S * 1000 + ncols)
    A = rng.standard_normal((S, ncols)) * np.exp(3 * rng.standard_normal(ncols))
    if steps == "uniform":
        T = np.arange(S) / 1000.0
    else:  # steps between 1e-4 and 1e-1, the extremes present
        dt = 10.0 ** rng.uniform(-4, -1, S)
        dt[[1, S - 2]] = 1e-4, 1e-1
        T = np.cumsum(dt)
    A.setflags(write=False)
    T.setflags(write=False)
    return A, T


@functools.lru_cache(maxsize=None)
def cd_reference(S, ncols, steps):
    """the exact differences as unevaluated sums hi + lo of two float64 (S, ncols) each, the bars (S, ncols) rounded up"""
    A, T = cd_input(S, ncols, steps)
    exact = [sr.central_diff(A[:, c], T) for c in range(ncols)]
    hi = np.array([sr.to_float(e) for e in exact]).T
    lo = np.array([[float(exact[c][t] - sr.mpf(float(hi[t, c]))) for c in range(ncols)] for t in range(S)])
    return hi, lo, cd_bar(A, T)


def cd_bar(A, T):
    """Entrywise rounding bar of the float64 central difference: 8 eps x the sum of the magnitudes of the terms of the numerator over the
    magnitude of the divisor (the edge rows: their two terms).  An interior entry has at most six roundings -- three additions (the
    scalings by 8 are exact), the difference of two time stamps, its product with 12, the quotient --, each relative to a partial
    result that the sum of magnitudes bounds; 8 covers them.  Derived, not measured.  (Evaluated in float64 and rounded up by 16 eps: it is a
    bar, not a reference.)"""
    S = A.shape[0]
    a = np.abs(A)
    div0, div_last = abs(T[1] - T[0]), abs(T[S - 3] - T[S - 4])
    bar = np.empty_like(A)
    bar[0] = (a[1] + a[0]) / div0
    bar[1] = (a[2] + a[0]) / (2 * div0)
    bar[2:S - 2] = (a[4:] + 8 * a[3:S - 1] + 8 * a[1:S - 3] + a[:S - 4]) / (12 * np.abs(T[2:S - 2] - T[1:S - 3]))[:, None]
    bar[S - 2] = (a[S - 1] + a[S - 3]) / (2 * div_last)
    bar[S - 1] = (a[S - 1] + a[S - 2]) / div_last
    return 8 * EPS * bar * (1 + 16 * EPS)


def cd_ratio(D, S, ncols, steps):
    """largest |D - exact| / bar over the entries (D - hi is exact where it matters: the two are within a factor of two)"""
    hi, lo, bar = cd_reference(S, ncols, steps)
    return float((np.abs((D - hi) - lo) / bar).max())


# ---- Data.preprocess ----------------------------------------------------------------------------------------------------------------------
PRE_CASES = [(Fs, k) for Fs in (1000.0, 2000.0) for k in (5, 31)]
PRE_OPT = {"useDeg": 0, "num_dofs": 2, "filterLowPass1": [8.0, 5], "filterLowPass2": [6.0, 5], "filterLowPass3": [3.0, 4], "waitForZeroAcc": 0,
           "zeroAccThresh": 0.1}
PRE_NAMES = ("Q", "V", "Vdot", "Tau")


@functools.lru_cache(maxsize=None)
def pre_input(Fs):
    rng = np.random.default_rng(int(Fs))
    S, n = 3000, 2
    T = np.arange(S) / Fs
    Q = np.sin(T[:, None] * (3.0 + 1.0 * np.arange(n))) + 0.01 * rng.standard_normal((S, n))
    Tau = 5 * np.cos(T[:, None] * (2.0 + 0.5 * np.arange(n))) + 0.3 * rng.standard_normal((S, n))
    for x in (T, Q, Tau):
        x.setflags(write=False)
    return Q, Tau, T


def pre_run(Fs, k, engine):
    """(Q, V, Vdot, Tau) of Data.preprocess with the given engine (None: the host SciPy pipeline)"""
    from flobaroid_amd.data import Data

    Q0, Tau0, T = pre_input(Fs)
    Q, V, Vdot, Tau = Q0.copy(), np.zeros_like(Q0), np.zeros_like(Q0), Tau0.copy()
    Data(dict(PRE_OPT, filterMedianSize=k)).preprocess(Q, V, Vdot, Tau, T.copy(), Fs, engine=engine)
    return Q, V, Vdot, Tau


@functools.lru_cache(maxsize=None)
def pre_reference(Fs, k):
    """exact chain per output: [n] channels of mpf; the deviations of the host SciPy pipeline from it; the bars (max over the channels of
    an output: 10 x the host's deviation, floor 64 eps max|want|)"""
    import scipy.signal as sig

    Q0, Tau0, T = pre_input(Fs)
    lp = [sig.butter(order, fc / (Fs / 2), btype="low", analog=False) for fc, order in (PRE_OPT["filterLowPass1"], PRE_OPT["filterLowPass2"])]
    exact = [sr.preprocess(Q0[:, j], Tau0[:, j], T, k, lp[0], lp[1]) for j in range(Q0.shape[1])]
    exact = {name: [exact[j][i] for j in range(Q0.shape[1])] for i, name in enumerate(PRE_NAMES)}
    host = dict(zip(PRE_NAMES, pre_run(Fs, k, None)))
    bars = {}
    for name in PRE_NAMES:
        scale = max(float(max(abs(v) for v in ch)) for ch in exact[name])
        bars[name] = max(10 * pre_deviation(host[name], exact[name]), 64 * EPS * scale)
    return exact, bars


def pre_deviation(got, exact_channels):
    return max(sr.deviation(got[:, j], exact_channels[j]) for j in range(len(exact_channels)))
