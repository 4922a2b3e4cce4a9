"""The signal conditioning of Data.preprocess restated exactly (mpmath, 50 digits): the yardstick of csrc/fbr_signal.h and of its g++
emulation (tests/emul/signal_emul.cpp).  Every function takes one channel as a sequence of float64 (taken exactly) or mpf values and
returns a list of mpf; no floating-point arithmetic of NumPy touches a value.

  filtfilt      scipy.signal.filtfilt(b, a, x): normalisation by a[0], odd extension with padlen = 3 * ncoef, start states zi * (first
                extended sample) with zi the closed form of lfilter_zi, the transposed direct-form-II recurrence forward and backward
  medfilt       scipy.signal.medfilt(x, k): the median of the window of k, zeros beyond the ends (sorted)
  central_diff  the five rules of Data._central_diff (the trailing two rows divide by T[S-3] - T[S-4])
  preprocess    the chain Data.preprocess applies to Q, V, Vdot and Tau
"""
import mpmath
from mpmath import mpf

DPS = 50
mpmath.mp.dps = DPS


def _exact(x):
    mpmath.mp.dps = DPS  # (another module may have changed the working precision)
    return [v if isinstance(v, mpf) else mpf(float(v)) for v in x]


def lfilter_zi(b, a):
    """Steady state of the transposed direct-form-II filter for a unit step, (b, a) normalised: the solution of (I - A) zi = B with A the
    companion matrix of a and B = b[1:] - a[1:] b[0], in closed form."""
    p = len(a) - 1
    B = [b[k] - a[k] * b[0] for k in range(1, p + 1)]
    zi = [sum(B) / sum(a)]
    for k in range(1, p):
        zi.append(sum(a[:k + 1]) * zi[0] - sum(B[:k]))
    return zi


def _lfilter(b, a, x, z):
    p = len(a) - 1
    z = list(z)
    y = []
    for u in x:
        v = z[0] + b[0] * u
        for i in range(p - 1):
            z[i] = z[i + 1] + u * b[i + 1] - v * a[i + 1]
        z[p - 1] = u * b[p] - v * a[p]
        y.append(v)
    return y


def filtfilt(b, a, x):
    b, a, x = _exact(b), _exact(a), _exact(x)
    n = max(len(a), len(b))
    b, a = b + [mpf(0)] * (n - len(b)), a + [mpf(0)] * (n - len(a))
    b, a = [v / a[0] for v in b], [v / a[0] for v in a]
    pad = 3 * n
    if len(x) <= pad:
        raise ValueError("the signal must be longer than the padding of 3 * ncoef samples")
    ext = [2 * x[0] - x[i] for i in range(pad, 0, -1)] + x + [2 * x[-1] - x[-1 - i] for i in range(1, pad + 1)]
    zi = lfilter_zi(b, a)
    y = _lfilter(b, a, ext, [v * ext[0] for v in zi])
    y = _lfilter(b, a, y[::-1], [v * y[-1] for v in zi])[::-1]
    return y[pad:len(y) - pad]


def medfilt(k, x):
    """Exact median of every window of k (odd) samples, zeros beyond the ends; the values themselves, no arithmetic."""
    if k < 1 or k % 2 == 0:
        raise ValueError("k must be odd")
    h = k // 2
    x = list(x)
    zero = mpf(0) if x and isinstance(x[0], mpf) else 0.0
    S = len(x)
    return [sorted([x[u] if 0 <= u < S else zero for u in range(t - h, t + h + 1)])[h] for t in range(S)]


def central_diff(a, t):
    a, t = _exact(a), _exact(t)
    S = len(a)
    if S < 5:
        raise ValueError("S >= 5")
    div0 = t[1] - t[0]
    div_last = t[S - 3] - t[S - 4]
    d = [None] * S
    d[0] = (a[1] - a[0]) / div0
    d[1] = (a[2] - a[0]) / (2 * div0)
    for i in range(2, S - 2):
        d[i] = (-a[i + 2] + 8 * a[i + 1] - 8 * a[i - 1] + a[i - 2]) / (12 * (t[i] - t[i - 1]))
    d[S - 2] = (a[S - 1] - a[S - 3]) / (2 * div_last)
    d[S - 1] = (a[S - 1] - a[S - 2]) / div_last
    return d


def preprocess(Q, Tau, T, k, lp1, lp2):
    """The chain of Data.preprocess on one joint: (Q, V, Vdot, Tau) from the position and torque channel, the time stamps, the median
    window k and the (b, a) of filterLowPass1 / filterLowPass2 (no IMU, no contact wrenches, useDeg 0)."""
    q = filtfilt(lp1[0], lp1[1], Q)
    v = filtfilt(lp2[0], lp2[1], medfilt(k, central_diff(q, T)))
    vdot = medfilt(k, central_diff(v, T))
    tau = filtfilt(lp1[0], lp1[1], medfilt(k, _exact(Tau)))
    return q, v, vdot, tau


def deviation(got, want):
    """max |got - want| over one channel as a float, the difference taken at the working precision"""
    mpmath.mp.dps = DPS
    return float(max(abs(mpf(float(g)) - w) for g, w in zip(got, want)))


def to_float(x):
    return [float(v) for v in x]
