"""NumPy restatement of the Jacobian of the trajectory series (classic Swevers and bounded tanh form, flobaroid_amd/csrc/fbr_kernels.h K6)
with respect to wf, q_offset, q_range, a_l, b_l -- closed forms for q, dq and ddq, written from the series themselves and checked against
SymPy's own ``diff`` in tests/test_dopt_gradient_host.py.  Works in any float type (``dtype=np.longdouble`` for the GPU comparisons).

With x_l = wf l t and wl = wf l:
  classic   q = q_offset + sum_l a_l sin(x_l) / wl - b_l cos(x_l) / wl,   dq = sum_l a_l cos(x_l) + b_l sin(x_l),   ddq = d(dq)/dt
  bounded   q = q_offset + q_range tanh(raw),  raw = sum_l b_l cos(x_l) + a_l sin(x_l),   dq, ddq its time derivatives
"""
import numpy as np


def series(wf, q_offset, q_range, a, b, t, dtype=np.float64):
    """q, dq, ddq (T,) of ONE joint."""
    t = np.asarray(t, dtype=dtype)
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    wf = dtype(wf)
    l = np.arange(1, a.size + 1).astype(dtype)
    wl = wf * l
    x = wf * (t[:, None] * l[None])
    sn, cs = np.sin(x), np.cos(x)
    if q_range is None:
        return dtype(q_offset) + sn @ (a / wl) - cs @ (b / wl), cs @ a + sn @ b, -sn @ (a * wl) + cs @ (b * wl)
    raw, rd, rdd = cs @ b + sn @ a, cs @ (a * wl) - sn @ (b * wl), -sn @ (a * wl**2) - cs @ (b * wl**2)
    th = np.tanh(raw)
    s2 = 1 - th**2
    qr = dtype(q_range)
    return dtype(q_offset) + qr * th, qr * s2 * rd, qr * (s2 * rdd - 2 * th * s2 * rd**2)


def series_jacobian(wf, q_range, a, b, t, dtype=np.float64):
    """Derivatives of ONE joint's (q, dq, ddq) over the samples t: an array (3, T, K), K = 3 + 2 nh, parameter order
    [wf, q_offset, q_range, a_1 .. a_nh, b_1 .. b_nh] (q_range column zero for the classic series)."""
    t = np.asarray(t, dtype=dtype)
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    wf = dtype(wf)
    nh, T = a.size, t.size
    l = np.arange(1, nh + 1).astype(dtype)
    wl = wf * l
    lt = t[:, None] * l[None]
    x = wf * lt
    sn, cs = np.sin(x), np.cos(x)
    J = np.zeros((3, T, 3 + 2 * nh), dtype=dtype)
    ia, ib = slice(3, 3 + nh), slice(3 + nh, 3 + 2 * nh)
    if q_range is None:
        J[0, :, 1] = 1
        J[0, :, ia], J[1, :, ia], J[2, :, ia] = sn / wl, cs, -wl * sn
        J[0, :, ib], J[1, :, ib], J[2, :, ib] = -cs / wl, sn, wl * cs
        # d/dwf: the amplitude 1 / wl and the phase x both move
        J[0, :, 0] = (lt * cs / wl - sn / (wf * wl)) @ a + (lt * sn / wl + cs / (wf * wl)) @ b
        J[1, :, 0] = (-lt * sn) @ a + (lt * cs) @ b
        J[2, :, 0] = -(l * sn + wl * lt * cs) @ a + (l * cs - wl * lt * sn) @ b
        return J
    qr = dtype(q_range)
    raw, rd, rdd = cs @ b + sn @ a, cs @ (a * wl) - sn @ (b * wl), -sn @ (a * wl**2) - cs @ (b * wl**2)
    th = np.tanh(raw)
    s2 = 1 - th**2

    def through_tanh(r0, r1, r2):
        """derivatives of (q, dq, ddq) for a parameter whose derivatives of (raw, rd, rdd) are (r0, r1, r2), each (T, k)"""
        T_, S_, RD, RDD = th[:, None], s2[:, None], rd[:, None], rdd[:, None]
        dq = qr * S_ * r0
        ddq = qr * (-2 * T_ * S_ * r0 * RD + S_ * r1)
        dddq = qr * (-2 * T_ * S_ * r0 * RDD + S_ * r2 - 2 * (S_ * (S_ - 2 * T_**2) * r0) * RD**2 - 4 * T_ * S_ * RD * r1)
        return dq, ddq, dddq

    J[0, :, ia], J[1, :, ia], J[2, :, ia] = through_tanh(sn, wl * cs, -(wl**2) * sn)
    J[0, :, ib], J[1, :, ib], J[2, :, ib] = through_tanh(cs, -wl * sn, -(wl**2) * cs)
    w0 = ((lt * cs) @ a - (lt * sn) @ b)[:, None]
    w1 = ((l * cs - wl * lt * sn) @ a - (l * sn + wl * lt * cs) @ b)[:, None]
    w2 = (-(2 * wl * l * sn + wl**2 * lt * cs) @ a - (2 * wl * l * cs - wl**2 * lt * sn) @ b)[:, None]
    for i, v in enumerate(through_tanh(w0, w1, w2)):
        J[i, :, 0] = v[:, 0]
    J[0, :, 1] = 1
    J[0, :, 2], J[1, :, 2], J[2, :, 2] = th, s2 * rd, s2 * rdd - 2 * th * s2 * rd**2
    return J


def chain(wf, q_range, A, B, sens_q, sens_dq, sens_ddq, t, dtype=np.longdouble):
    """Gradient of ONE candidate in the layout of fbr_fourier_gradient, [wf | q_offset (n) | q_range (n) | a (n, nh) | b (n, nh)], and, entry
    by entry, the sum over the samples of |sens_q dq/dp| + |sens_dq d(dq)/dp| + |sens_ddq d(ddq)/dp| (what a rounding bound scales with).
    A, B (n, nh); sens_* (T, n); q_range (n,) or None."""
    n, nh = np.asarray(A).shape
    g = np.zeros(1 + 2 * n + 2 * n * nh, dtype=dtype)
    mag = np.zeros_like(g)
    S = [np.asarray(s, dtype=dtype) for s in (sens_q, sens_dq, sens_ddq)]
    for j in range(n):
        J = series_jacobian(wf, None if q_range is None else q_range[j], A[j], B[j], t, dtype)
        terms = np.stack([S[i][:, j, None] * J[i] for i in range(3)])  # (3, T, K)
        v, m = terms.sum(axis=(0, 1)), np.abs(terms).sum(axis=(0, 1))
        idx = np.concatenate([[0, 1 + j, 1 + n + j], 1 + 2 * n + j * nh + np.arange(nh), 1 + 2 * n + n * nh + j * nh + np.arange(nh)])
        np.add.at(g, idx, v)
        np.add.at(mag, idx, m)
    return g, mag
