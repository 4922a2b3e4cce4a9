"""Two rhs columns through the Gram pass over sample-contiguous images (csrc/fbr_gram64.h), without a GPU.

The producer keeps, per workgroup and lane, one running sum per (column, rhs column) and one per entry of the upper triangle of
rhs^T W^2 rhs (fbr_gram64_mom_count); fbr_gram64_mom_reduce_kernel adds them up and writes them where fbr_gram64_mom_target says.
tests/emul/gram64_rhs.cpp walks that accumulation and that index map from the SAME host tables (fbr_gram64_build +
fbr_gram64_build_producer); here its Gram is compared with the oracle's A^T A, A = [Y | rhs], for k = 2 on the shipped robots and on
random trees, and every running sum is checked to have exactly one writer per lane and block -- what makes the pass reproducible to
the bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from common import load_topo, random_states, random_topology
from oracle.oracle import OracleModel

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "gram64_rhs.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libgram64_rhs.so")
_lib = None
_dp = ctypes.POINTER(ctypes.c_double)


def lib():
    global _lib
    if _lib is None:
        import emul_lib

        deps = [_SRC, emul_lib._SRC, os.path.join(emul_lib._CSRC, "fbr_gram64.h"), os.path.join(emul_lib._CSRC, "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            tmp = f"{_OUT}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, _SRC])
            os.replace(tmp, _OUT)
        _lib = ctypes.CDLL(_OUT)
    return _lib


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def gram64_rhs(em, st, rhs, w=None, sign=None, force_tiles=True):
    """(G, stats) of the emulated pass with the rhs columns ``rhs`` [S rows][k], or None when the model is outside the pass"""
    S, q, dq, ddq, bv, ba, rpy = em._st(st)
    rhs = np.ascontiguousarray(rhs, dtype=np.float64).reshape(S * em.rows, -1)
    k = rhs.shape[1]
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    sign = None if sign is None else np.ascontiguousarray(sign, dtype=np.float64)
    G = np.zeros((em.cols + k, em.cols + k))
    ws = (ctypes.c_long * 5)()
    rc = lib().gram64_rhs(ctypes.byref(em.t), ctypes.c_long(S), _d(q), _d(dq), _d(ddq), _d(bv), _d(ba), _d(rpy), _d(sign), _d(rhs), int(k), _d(w),
                          int(force_tiles), _d(G), ws)
    if rc == -1:
        return None
    assert rc == 0, rc
    return G, dict(zip(("min_writers", "max_writers", "max_writers_untiled", "tiled_columns", "sums"), (int(v) for v in ws)))


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _check(em, E, om, st, rhs, w, sign=None, force_tiles=True):
    """the emulated Gram of the (reduced) model ``em``, expanded by E, against the oracle's; False: the model is outside the pass"""
    k = rhs.shape[1]
    got = gram64_rhs(em, st, rhs, w, sign, force_tiles)
    if got is None:
        return False
    G, ws = got
    assert ws["sums"] == k * em.cols + k * (k + 1) // 2
    assert ws["min_writers"] == 1 and ws["max_writers"] == 1, ws  # one adder per address
    assert ws["max_writers_untiled"] == 0, ws  # (a structurally zero column has no products)
    Y = om.regressor(st, sign)
    A = np.hstack([Y, rhs])
    if w is not None:
        A = A * w[:, None]
    Ea = np.zeros((em.cols + k, om.P + k))
    Ea[: em.cols, : om.P] = E
    Ea[em.cols:, om.P:] = np.eye(k)
    assert _rel(Ea.T @ G @ Ea, A.T @ A) <= 1e-12
    assert np.array_equal(G, G.T)
    # the rhs columns sit where they belong: column P + i of G is Y^T W^2 rhs_i
    W2 = 1.0 if w is None else (w * w)[:, None]
    for i in range(k):
        ref = (Y * W2).T @ rhs[:, i]
        assert np.linalg.norm(E.T @ G[: em.cols, em.cols + i] - ref) <= 1e-12 * max(np.linalg.norm(A.T @ A), 1e-300)
    return True


def test_index_map_covers_the_rhs_block_once():
    """fbr_gram64_mom_target for k = 1 is the layout the one-column pass had ([cols] products, then tau^T tau); for k = 2 every entry of
    the upper triangle of the rhs block of G is hit by exactly one running sum (gram64_rhs returns an error otherwise)."""
    import emul_lib

    t = load_topo("threeLinks")
    em = emul_lib.Emul(t, floating=False)
    rng = np.random.default_rng(5)
    st = random_states(t, 3, rng, False)
    for k in (1, 2):
        got = gram64_rhs(em, st, rng.standard_normal((3 * em.rows, k)))
        assert got is not None and got[1]["sums"] == k * em.cols + (1, 3)[k - 1]
    assert gram64_rhs(em, st, rng.standard_normal((3 * em.rows, 3))) is None  # k = 3 stays on the per-sample-image pass


@pytest.mark.parametrize("case,floating,which,fric", [("walkman_apriori", True, 1, False), ("walkman_left_arm", True, -1, False),
                                                     ("walkman_left_arm", True, 1, False), ("walkman_left_arm", True, -1, True),
                                                     ("kuka_lwr4", False, -1, False), ("kuka_lwr4", False, -1, True),
                                                     ("threeLinks", True, -1, False)])
@pytest.mark.parametrize("weights", [False, True], ids=["plain", "weights"])
def test_two_rhs_columns_on_shipped_robots(case, floating, which, fric, weights):
    import emul_lib

    rng = np.random.default_rng(91)
    t = load_topo(case)
    om = OracleModel(t, floating=floating, fric=fric, fric_sym=True)
    em = emul_lib.Emul(t, floating=floating, fric=fric)
    E = np.eye(om.P)
    if which >= 0:
        em, E = em.reduction(which)
    S = 64 + 13
    st = random_states(t, S, rng, floating)
    sign = np.tanh(st["dq"] / 0.02) if fric else None
    rhs = rng.standard_normal((S * om.rows, 2))
    rhs[:, 1] *= 1e3  # (columns of very different scale: a mix-up shows)
    w = 0.5 + rng.random(S * om.rows) if weights else None
    assert _check(em, E, om, st, rhs, w, sign), "the shipped robots' one-part programs are inside the pass"
    assert _check(em, E, om, st, rhs, w, sign, force_tiles=False)
    rhs[:, 1] = 0.0  # the common contactForcesSum
    assert _check(em, E, om, st, rhs, w, sign)


def test_two_part_program_stays_outside():
    import emul_lib

    t = load_topo("walkman_apriori")
    em = emul_lib.Emul(t, floating=True)
    rng = np.random.default_rng(3)
    st = random_states(t, 2, rng, True)
    assert gram64_rhs(em, st, rng.standard_normal((2 * em.rows, 2))) is None


@pytest.mark.parametrize("seed", range(10))
def test_two_rhs_columns_on_random_trees(seed):
    import emul_lib

    rng = np.random.default_rng(4100 + seed)
    t = random_topology(rng, 6 + 5 * (seed % 4), p_fixed=0.3, branchiness=0.5, p_prismatic=0.3 if seed % 3 == 0 else 0.0)
    if t.num_dofs == 0:
        pytest.skip("no joints")
    floating, fric = seed % 2 == 0, seed % 3 == 1
    om = OracleModel(t, floating=floating, fric=fric, fric_sym=True)
    em = emul_lib.Emul(t, floating=floating, fric=fric)
    S = 64 + 5 + seed
    st = random_states(t, S, rng, floating)
    sign = np.tanh(st["dq"] / 0.02) if fric else None
    rhs = rng.standard_normal((S * om.rows, 2))
    w = 0.5 + rng.random(S * om.rows) if seed % 2 else None
    # the pass serves two rhs columns wherever it serves one (the emulation of the one-column pass: emul_lib.Emul.gram64)
    for cand, E in [(em, np.eye(om.P))] + [r for r in (em.reduction(1),) if r is not None]:
        one = cand.gram64(st, rhs[:, :1], w, sign) is not None
        assert _check(cand, E, om, st, rhs, w, sign) == one

