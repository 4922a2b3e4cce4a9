"""The run tables of the Gram kernel's pipelined slot walk (csrc/fbr_gram64.h, FbrGram64::runs), without a GPU.

In the 8 x 18 shape every wave orders its tile pairs so that the pairs a level takes part in are consecutive slots [qa, qb); the kernel
then reads the next slot's operands while the current slot's MFMAs run.  Checked on the shipped robots (all columns, merged, regrouped;
with and without friction and force tiles) and on random trees: every pair in exactly one slot, the run of every (wave, level) exactly
the slots active there, the tables present on the robot bench.py measures, and the Gram of the emulated pass still the oracle's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from common import load_topo, random_topology, random_states
from oracle.oracle import OracleModel

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "gram64_runs.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libgram64_runs.so")
_lib = None


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


def tables(em, k=1, force_tiles=True):
    """(waves, slots, levels, tiles, wmeta [waves][slots][3], runs [waves][levels] or None), or None outside the pass"""
    cap = 1 << 16
    dims = np.zeros(5, np.int32)
    wmeta = np.zeros(cap, np.int32)
    runs = np.zeros(cap, np.int32)
    ip = ctypes.POINTER(ctypes.c_int32)
    rc = lib().gram64_runs(ctypes.byref(em.t), int(k), int(force_tiles), dims.ctypes.data_as(ip), wmeta.ctypes.data_as(ip),
                           runs.ctypes.data_as(ip), ctypes.c_long(cap))
    if rc == -1:
        return None
    assert rc == 0
    W, npw, nlev, ntiles, has = (int(x) for x in dims)
    return W, npw, nlev, ntiles, wmeta[: W * npw * 3].reshape(W, npw, 3), runs[: W * nlev].reshape(W, nlev) if has else None


def check(tb):
    """every pair in exactly one slot, the run of every (wave, level) exactly its active slots; True when the runs are there"""
    W, npw, nlev, ntiles, wm, runs = tb
    seen = set()
    for w in range(W):
        for q in range(npw):
            I, J, r = (int(x) for x in wm[w, q])
            if I < 0:
                continue
            lo, hi = r & 0xFF, r >> 8
            assert 0 <= I < ntiles and 0 <= J < ntiles and 0 <= lo < hi <= nlev
            key = (min(I, J), max(I, J))
            assert key not in seen, ("pair in two slots", key)
            seen.add(key)
    if runs is None:
        return False
    assert W == 8 and npw > 10  # (only the 8 x 18 shape pipelines its slots)
    for w in range(W):
        for lv in range(nlev):
            qa, qb = int(runs[w, lv]) & 0xFF, int(runs[w, lv]) >> 8
            assert 0 <= qa <= qb <= npw
            act = [q for q in range(npw) if wm[w, q, 0] >= 0 and (wm[w, q, 2] & 0xFF) <= lv < (wm[w, q, 2] >> 8)]
            assert act == list(range(qa, qb)) or (not act and qa == qb), (w, lv, act, qa, qb)
    return True


def models():
    out = []
    for case, floating in (("walkman_apriori", True), ("walkman_left_arm", True), ("kuka_lwr4", False), ("threeLinks", False)):
        for fric in (False, True):
            out.append((case, floating, fric))
    return out


@pytest.mark.parametrize("case,floating,fric", models())
@pytest.mark.parametrize("which", [-1, 0, 1], ids=["all_columns", "merged", "regrouped"])
def test_runs_on_shipped_robots(case, floating, fric, which):
    import emul_lib

    t = load_topo(case)
    em = emul_lib.Emul(t, floating=floating, fric=fric)
    if which >= 0:
        red = em.reduction(which)
        if red is None:
            pytest.skip("nothing to reduce")
        em = red[0]
    for k in (0, 1):
        for ft in (True, False):
            tb = tables(em, k, ft)
            if tb is None:
                continue
            has = check(tb)
            if case == "walkman_apriori" and which == 1 and not fric:
                assert has, "the robot bench.py measures runs the pipelined walk"


@pytest.mark.parametrize("seed", range(12))
def test_runs_on_random_trees(seed):
    import emul_lib

    rng = np.random.default_rng(1300 + seed)
    t = random_topology(rng, 10 + 6 * (seed % 4), p_fixed=0.3, branchiness=0.5, p_prismatic=0.3 if seed % 3 == 0 else 0.0)
    if t.num_dofs == 0:
        pytest.skip("no joints")
    for fric in (False, True):
        em = emul_lib.Emul(t, floating=seed % 2 == 0, fric=fric)
        for cand in [em] + [r[0] for r in (em.reduction(1),) if r is not None]:
            tb = tables(cand, 1)
            if tb is not None:
                check(tb)


@pytest.mark.parametrize("case,which", [("walkman_apriori", 1), ("walkman_left_arm", 1), ("kuka_lwr4", -1)])
def test_emulated_gram_with_runs(case, which):
    """the emulated pass (the same host tables, slots reordered) still computes the oracle's [Y | tau] Gram"""
    import emul_lib

    rng = np.random.default_rng(77)
    t = load_topo(case)
    floating = case != "kuka_lwr4"
    om = OracleModel(t, floating=floating)
    em = emul_lib.Emul(t, floating=floating)
    E = np.eye(om.P)
    if which >= 0:
        em, E = em.reduction(which)
    S = 70
    st = random_states(t, S, rng, floating)
    Y = om.regressor(st, None)
    tau = rng.standard_normal((Y.shape[0], 1))
    w = rng.random(Y.shape[0]) + 0.5
    got = em.gram64(st, tau, w)
    assert got is not None
    Gr, _ = got
    Ea = np.zeros((em.cols + 1, om.P + 1))
    Ea[: em.cols, : om.P] = E
    Ea[-1, -1] = 1.0
    A = np.hstack([Y, tau]) * w[:, None]
    assert np.linalg.norm(Ea.T @ Gr @ Ea - A.T @ A) <= 1e-12 * np.linalg.norm(A.T @ A)
    assert np.array_equal(Gr, Gr.T)
