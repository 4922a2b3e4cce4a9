"""Column-scaled bars for the Gram pass and the TSQR (test helper, not shipped).

A Frobenius ratio ``norm(G - G_ref) / norm(G_ref)`` is blind to the small columns of the regressor: an entry that involves one is 1e4 to
1e14 x smaller than the norm.  The metric here judges every entry on the scale of its own two columns.  For a reference Gram
``G_ref = A^T A`` in long double, ``A = [Y | rhs]`` and ``d_j = sqrt(G_ref[j, j])``::

    dt_j = max(d_j, theta * max over the Y columns of d)   for a column of Y
    dt_j = d_j                                             for an rhs column (inputs are exact: no floor)
    m_theta(G) = max_ij |G_ij - G_ref,ij| / (dt_i dt_j)    evaluated in long double

The floor exists for one reason: a fixed-base robot has regressor columns that are zero (kuka_lwr4: 20 of 108 exactly, more as rounding
residue of about 1e-20 of the largest), and in double arithmetic such a column is 1e-17-sized noise whose error, divided by its own norm,
reads 1e6.  theta = 1e-2 judges every column within 100 x of the largest on its own scale, theta = 1e-4 every column within 1e4 x.

The bar of a device call, on the same inputs, with N stacked rows of nonzero weight::

    bar_theta = 16 * max over the CPU routes of m_theta  +  N * 2^-53

The CPU routes are plain double arithmetic in other summation orders (the double oracle's regressor, the emulation of the kernels'
regressor, the emulation's reduced robots expanded through E; for a factor also LAPACK's Householder R of the oracle's matrix); 16 is the
"8 x the oracle" of edge_reference.class_bar doubled, since the routes differ in summation order only.  N u d_i d_j bounds a sum of N
products taken in any order (gamma_N sum |a_i| |a_j| <= N u d_i d_j): MFMA k-steps, chunk partials and atomics alike.  For a factor it is
an allowance, stricter than Householder's proven constant.  tests/test_colscale_reference.py caps the CPU routes themselves (CAP), so the
device bar cannot grow with them unseen.  No number here comes from the device.

Everything is built on edge_reference.reference(key) and its classes, unchanged.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import edge_reference as er

LD = np.longdouble
T = er.CLASS_SIZE
U = 2.0 ** -53
THETAS = (1e-2, 1e-4)
CAP = {1e-2: 1.5e-14, 1e-4: 2.5e-13}   # about twice the worst m_theta of any CPU route, any configuration and class
ROUTE_FACTOR = 16.0
SIZES = (1, 11)                        # a class's own 24 samples, and the class tiled to 264
LS_KEYS = ("walkman_left_arm-fb-fric", "tree12-fb")
LS_CLASSES = ("ordinary", "fast", "hardacc")
LS_RANK_TOL = 1e-9
LS_FACTOR = 16.0


# ------------------------------------------------------------------------------------------------------------------------------------
# the metric
# ------------------------------------------------------------------------------------------------------------------------------------
def column_scales(Gref, nY, theta):
    """dt (n,) in long double: floored for the first nY columns (the regressor's), the plain d_j for the rhs columns behind them"""
    d = np.sqrt(np.diag(np.asarray(Gref, dtype=LD)))
    dt = d.copy()
    if nY > 0:
        dt[:nY] = np.maximum(d[:nY], LD(theta) * d[:nY].max())
    return dt


def metric(G, Gref, theta, nY):
    """m_theta(G) against G_ref, whose first nY columns are the regressor's.  An rhs column with d_j = 0 is not used; an entry whose scale
    is 0 (theta = 0 and a zero column) counts 0 when it is matched exactly and inf otherwise."""
    Gref = np.asarray(Gref, dtype=LD)
    dt = column_scales(Gref, nY, theta)
    use = np.ones(dt.size, dtype=bool)
    use[nY:] = dt[nY:] > 0
    diff = np.abs(np.asarray(G, dtype=LD) - Gref)[np.ix_(use, use)]
    den = np.outer(dt[use], dt[use])
    pos = den > 0
    r = np.where(pos, diff / np.where(pos, den, LD(1)), np.where(diff > 0, LD(np.inf), LD(0)))
    return float(r.max()) if r.size else 0.0


def frobenius_ratio(G, Gref):
    """the suite's coarse net: norm(G - G_ref) / norm(G_ref) in long double"""
    Gref = np.asarray(Gref, dtype=LD)
    return float(np.sqrt(((np.asarray(G, dtype=LD) - Gref) ** 2).sum()) / np.sqrt((Gref ** 2).sum()))


# ------------------------------------------------------------------------------------------------------------------------------------
# long-double linear algebra (a few hundred rows by about 120 columns: plain loops)
# ------------------------------------------------------------------------------------------------------------------------------------
def householder_ld(A, pivot=False):
    """Householder QR in long double: the upper-triangular R (n, n) of A (m, n), m >= n; with ``pivot`` also the column order (the largest
    remaining column first), R then being the factor of A[:, order]."""
    A = np.array(A, dtype=LD)
    m, n = A.shape
    assert m >= n
    order = np.arange(n)
    for j in range(n):
        if pivot:
            p = j + int(np.argmax((A[j:, j:] ** 2).sum(axis=0)))
            if p != j:
                A[:, [j, p]] = A[:, [p, j]]
                order[[j, p]] = order[[p, j]]
        x = A[j:, j]
        s = np.sqrt((x * x).sum())
        if s == 0:
            continue
        alpha = -s if x[0] >= 0 else s
        v = x.copy()
        v[0] -= alpha
        v /= np.sqrt((v * v).sum())
        A[j:, j:] -= LD(2) * np.outer(v, v @ A[j:, j:])
        A[j, j] = alpha
        A[j + 1:, j] = 0
    R = np.triu(A[:n])
    return (R, order) if pivot else R


def back_substitute(R, b):
    """x with R x = b for an upper-triangular R, in the dtype of R"""
    n = R.shape[0]
    x = np.zeros(n, dtype=R.dtype)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - R[i, i + 1:] @ x[i + 1:]) / R[i, i]
    return x


def rtr(R):
    """R^T R in long double"""
    R = np.asarray(R, dtype=LD)
    return R.T @ R


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs of one configuration, shared by every test and left unchanged
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(key: str):
    """rhs (S, rows, 2): N(0, 1) x the class's own max|Y_ref| in the first column, 1e-6 x that in the second; row weights (S, rows) drawn
    from {0, 0.5, 1, 2} (their products with a double are exact); a column subset (about two thirds of the columns, in order)."""
    ref = er.reference(key)
    rng = np.random.default_rng([81, er.CONFIG_KEYS.index(key)])
    rhs = rng.standard_normal((ref["S"], ref["rows"], 2))
    for sl in er.class_slices(ref["names"]).values():
        rhs[sl] *= float(np.abs(ref["Y"][sl]).max())
    rhs[:, :, 1] *= 1e-6
    w = rng.choice(np.array([0.0, 0.5, 1.0, 2.0]), size=(ref["S"], ref["rows"]))
    cols = np.sort(rng.choice(ref["P"], size=(2 * ref["P"]) // 3, replace=False)).astype(np.int32)
    for a in (rhs, w, cols):
        a.setflags(write=False)
    return {"rhs": rhs, "w": w, "cols": cols}


@functools.lru_cache(maxsize=None)
def cpu_regressors(key: str):
    """The double regressors of the CPU routes over the whole edge batch: name -> (Y (S * rows, P_route), E (P_route, P) or None).
    oracle: oracle/fbr_oracle.c; emulation: the kernels' own arithmetic (tests/emul_lib.Emul.regressor); reduced0 / reduced1: the
    emulation of the reduced robots the library runs its passes on (fixed links merged; merged and regrouped), Y = Y_red E."""
    from emul_lib import Emul
    from oracle.oracle import OracleModel

    topo, floating, friction, stribeck = er.config(key)
    ref = er.reference(key)
    est = er.engine_states(ref["st"])
    sign = est.get("sign")
    om = OracleModel(topo, floating=floating, fric=friction, fric_sym=True, stribeck=stribeck)
    em = Emul(topo, floating=floating, fric=friction, fric_sym=True, stribeck=stribeck)
    out = {"oracle": (om.regressor(est, sign), None), "emulation": (em.regressor(est, sign), None)}
    for which in (0, 1):
        red = em.reduction(which)
        if red is not None:
            out[f"reduced{which}"] = (red[0].regressor(est, sign), red[1])
    for Y, E in out.values():
        Y.setflags(write=False)
    return out


class Call(NamedTuple):
    """one Gram or factor: the classes stacked, each tiled ``rep`` times, k rhs columns, row weights or none, the column subset or all"""
    classes: tuple
    rep: int = 1
    k: int = 0
    weighted: bool = False
    subset: bool = False
    factor: bool = False   # a TSQR result: the CPU routes then include LAPACK's R


def _rows_of(key, classes):
    ref = er.reference(key)
    sl = er.class_slices(ref["names"])
    rows = ref["rows"]
    return np.concatenate([np.arange(sl[c].start * rows, sl[c].stop * rows) for c in classes])


@functools.lru_cache(maxsize=None)
def _class_gram_ld(key, cls, weighted):
    """the long-double A^T A of one class, A = [Y | both rhs columns] (x the row weights)"""
    ref = er.reference(key)
    idx = _rows_of(key, (cls,))
    A = np.concatenate([ref["Y"].reshape(-1, ref["P"])[idx], np.asarray(inputs(key)["rhs"].reshape(-1, 2)[idx], dtype=LD)], axis=1)
    if weighted:
        A = A * np.asarray(inputs(key)["w"].reshape(-1)[idx], dtype=LD)[:, None]
    return A.T @ A


def _select(key, call):
    P = er.reference(key)["P"]
    cols = inputs(key)["cols"] if call.subset else np.arange(P)
    return cols, np.concatenate([cols, P + np.arange(call.k)])


def reference_gram(key, call: Call):
    """(G_ref in long double, the number of regressor columns in it)"""
    cols, sel = _select(key, call)
    G = sum(_class_gram_ld(key, c, call.weighted) for c in call.classes)
    return LD(call.rep) * G[np.ix_(sel, sel)], cols.size


def nonzero_rows(key, call: Call):
    idx = _rows_of(key, call.classes)
    return call.rep * (int(np.count_nonzero(inputs(key)["w"].reshape(-1)[idx])) if call.weighted else idx.size)


def cpu_grams(key, call: Call):
    """name -> the Gram of every CPU route on the inputs of the call, in double (R^T R of LAPACK's factor in long double)"""
    P = er.reference(key)["P"]
    cols, sel = _select(key, call)
    idx = _rows_of(key, call.classes)
    rhs = inputs(key)["rhs"].reshape(-1, 2)[idx][:, :call.k]
    w = inputs(key)["w"].reshape(-1)[idx][:, None] if call.weighted else 1.0
    out = {}
    for name, (Y, E) in cpu_regressors(key).items():
        A = np.tile(np.hstack([Y[idx], rhs]) * w, (call.rep, 1))
        G = A.T @ A
        if E is not None:
            Ea = np.zeros((E.shape[0] + call.k, P + call.k))
            Ea[:E.shape[0], :P] = E
            Ea[E.shape[0]:, P:] = np.eye(call.k)
            G = Ea.T @ G @ Ea
            out[name] = G[np.ix_(sel, sel)]
        else:
            out[name] = G if not call.subset else G[np.ix_(sel, sel)]
            if name == "oracle" and call.factor:
                out["lapack"] = rtr(np.linalg.qr(A[:, sel], mode="r"))
    return out


@functools.lru_cache(maxsize=None)
def cpu_metrics(key, call: Call):
    """route -> {theta: m_theta} of the CPU routes on the inputs of the call"""
    Gref, nY = reference_gram(key, call)
    return {name: {th: metric(G, Gref, th, nY) for th in THETAS} for name, G in cpu_grams(key, call).items()}


def cap(key, call: Call):
    """{theta: the most a CPU route may read on the inputs of the call}: CAP for a class's own 24 samples; a tiled or merged call is a
    longer sum in double, and what it may add is the worst-case N u of the rows beyond those 24 samples"""
    extra = max(0, nonzero_rows(key, call) - T * er.reference(key)["rows"]) * U
    return {th: CAP[th] + extra for th in THETAS}


def bar(key, call: Call):
    """{theta: bar_theta} of a device call on these inputs"""
    m = cpu_metrics(key, call)
    n = nonzero_rows(key, call)
    return {th: ROUTE_FACTOR * max(r[th] for r in m.values()) + n * U for th in THETAS}


def device_calls(key):
    """what -> [(label, Call)]: every call tests/test_gpu_colscale.py makes, class by class and at both sizes.  The accumulated Gram and
    the factor streamed through R_in see the inputs of the one-call Gram / factor, split in two halves; a merge joins the factors of a
    class and of the class behind it (the last with the first)."""
    names = er.reference(key)["names"]
    behind = {c: names[(i + 1) % len(names)] for i, c in enumerate(names)}
    out = {}
    for rep in SIZES:
        each = lambda **kw: [(c, Call((c,), rep, **kw)) for c in names]  # noqa: E731
        S = f"S={T * rep}"
        out[f"gram k=0 {S}"] = each(k=0)
        out[f"gram k=1 {S}"] = each(k=1)
        out[f"gram k=2 {S}"] = each(k=2)
        out[f"gram weights {S}"] = each(k=1, weighted=True)
        out[f"gram accumulate {S}"] = each(k=1)
        out[f"gram_grouped {S}"] = each(k=2)
        out[f"tsqr {S}"] = each(k=2, factor=True)
        out[f"tsqr weights {S}"] = each(k=1, weighted=True, factor=True)
        out[f"tsqr R_in {S}"] = each(k=2, factor=True)
        out[f"tsqr cols {S}"] = each(k=1, subset=True, factor=True)
        out[f"tsqr_merge {S}"] = [(f"{c}+{behind[c]}", Call((c, behind[c]), rep, k=2, factor=True)) for c in names]
    return out


def call_states(key, call: Call):
    """(engine states, rhs (N, k) or None, w (N,) or None, cols or None) of a call: what the device is handed"""
    ref = er.reference(key)
    sl = er.class_slices(ref["names"])
    sample = np.concatenate([np.tile(np.arange(sl[c].start, sl[c].stop), call.rep) for c in call.classes])
    st = er.engine_states(er.sample_states(ref["st"], sample))
    rhs = np.ascontiguousarray(inputs(key)["rhs"][sample][:, :, :call.k].reshape(-1, call.k)) if call.k else None
    w = np.ascontiguousarray(inputs(key)["w"][sample].reshape(-1)) if call.weighted else None
    return st, rhs, w, (inputs(key)["cols"] if call.subset else None)


# ------------------------------------------------------------------------------------------------------------------------------------
# least squares: a factor of Householder quality, not of Cholesky quality
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ls_case(key, cls):
    """The least-squares problem of one class over its independent columns.  Columns: pivoted Householder QR of the column-normalised
    long-double Y, rank by |r_jj| > 1e-9 |r_11|.  rhs: the first rhs column of ``inputs``.  x_ref comes from the long-double Householder
    factor of [Y[:, cols] | rhs].  -> cols, d (the columns' norms), x_ref, e_qr (LAPACK's QR of the oracle's double matrix), e_chol
    (normal equations + Cholesky in double)."""
    ref = er.reference(key)
    idx = _rows_of(key, (cls,))
    Y = ref["Y"].reshape(-1, ref["P"])[idx]
    dall = np.sqrt((Y * Y).sum(axis=0))
    R, order = householder_ld(Y / np.where(dall > 0, dall, LD(1)), pivot=True)
    diag = np.abs(np.diag(R))
    cols = np.sort(order[diag > LS_RANK_TOL * diag[0]]).astype(np.int32)
    r = cols.size
    rhs = inputs(key)["rhs"].reshape(-1, 2)[idx][:, :1]
    Rl = householder_ld(np.concatenate([Y[:, cols], np.asarray(rhs, dtype=LD)], axis=1))
    x_ref = back_substitute(Rl[:r, :r], Rl[:r, r])
    d = dall[cols]
    A = np.hstack([cpu_regressors(key)["oracle"][0][idx][:, cols], rhs])
    Rq = np.linalg.qr(A, mode="r")
    G = A.T @ A
    Rc = np.linalg.cholesky(G[:r, :r]).T
    x_chol = back_substitute(Rc, back_substitute(Rc.T[::-1, ::-1], G[:r, r][::-1])[::-1])
    return {"cols": cols, "d": d, "x_ref": x_ref, "e_qr": ls_error(solve_factor(Rq, r), x_ref, d), "e_chol": ls_error(x_chol, x_ref, d)}


def solve_factor(R, r):
    """x = R[:r, :r]^-1 R[:r, r] of a factor of [Y[:, cols] | rhs], in double"""
    R = np.asarray(R, dtype=np.float64)
    return back_substitute(R[:r, :r], R[:r, r])


def ls_error(x, x_ref, d):
    """e = max_j |x_j - x_ref,j| d_j / max_j |x_ref,j| d_j in long double"""
    return float((np.abs(np.asarray(x, dtype=LD) - x_ref) * d).max() / (np.abs(x_ref) * d).max())
