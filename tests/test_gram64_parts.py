"""The producer's parts and the chunk sizes of the sample-contiguous Gram pass (csrc/fbr_gram64.h: fbr_gram64_build_producer with the
options gram_lane_skip_unowned and gram_lane_parts_cut, fbr_gram64_chunk_plan with gram_lane_chunk_rounds), without a GPU.

Checked by tests/emul/gram64_parts.cpp on the shipped robots (all columns, merged, regrouped; with and without friction) and on random
trees, for the present cut (0) and the new one (1): every inertial and friction column that has a tile has exactly one owning part, a
part's walked set is closed under parents and holds every link it writes, the owns-nothing flag is set exactly where all 18 destination
words are zero and all lane columns are -1, the new cut's modelled slowest part is never above the present cut's, and the cut repeats.
The emulated pass (emul_gram64 builds the image from the destination words alone, so a link without words is not visited; it takes the
default cut, the present one -- the new cut's tables go through the checks above, and its bits are compared on the GPU) still gives the
oracle's Gram."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from common import load_topo, random_topology, random_states
from oracle.oracle import OracleModel

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "gram64_parts.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libgram64_parts.so")
_lib = None
_COLS = ("steps", "links", "entries", "unowned", "discarded", "cost")


def lib():
    global _lib
    if _lib is None:
        import emul_lib

        deps = [_SRC, emul_lib._SRC] + [os.path.join(emul_lib._CSRC, h) for h in ("fbr_gram64.h", "fbr_program.h", "fbr_kinid.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            tmp = f"{_OUT}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, _SRC])
            os.replace(tmp, _OUT)
        _lib = ctypes.CDLL(_OUT)
    return _lib


def parts(em, k, cut, force=None):
    """(per-part table of _COLS, cut points, checksum of the producer's tables) or None outside the pass; the checks of
    gram64_parts.cpp have passed"""
    st = np.zeros((4, 6))
    starts = np.zeros(5, np.int32)
    fc = np.asarray([-1] * 5 if force is None else force, np.int32)
    h = ctypes.c_ulonglong(0)
    rc = lib().gram64_parts(ctypes.byref(em.t), int(k), int(cut), fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                            st.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), starts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(h))
    if rc == -1:
        return None
    assert rc >= 1, f"check {rc} of gram64_parts.cpp failed"
    return st[:rc], [int(x) for x in starts[: rc + 1]], h.value


def check_model(em, k):
    old, new = parts(em, k, 0), parts(em, k, 1)
    assert (old is None) == (new is None)
    if old is None:
        return None
    for cut, ref in ((0, old), (1, new)):
        again = parts(em, k, cut)
        assert again[1] == ref[1] and again[2] == ref[2], "the cut does not repeat"
    assert new[0][:, 5].max() <= old[0][:, 5].max(), "the new cut's slowest part is dearer than the present cut's"
    assert new[0][:, 2].sum() == old[0][:, 2].sum() and new[0][:, 1].sum() == old[0][:, 1].sum()  # the same links and entries, dealt otherwise
    # a forced cut (how the coefficients are measured) goes through the same checks
    forced = parts(em, k, 0, force=new[1] + [new[1][-1]] * (5 - len(new[1])))
    if len(new[1]) == 5:
        assert forced[1] == new[1] and forced[2] == new[2]
    return old, new


def models():
    out = []
    for case, floating in (("walkman_apriori", True), ("walkman_left_arm", True), ("kuka_lwr4", False), ("threeLinks", False)):
        for fric in (False, True):
            out.append((case, floating, fric))
    return out


# regrouped walkman_apriori, k = 1 (the model bench.py measures): steps walked, owned links, owned entries, unowned links walked,
# entries of those (what the producer formed and discarded before gram_lane_skip_unowned)
WALKMAN_OLD = [[8, 8, 508, 0, 0], [11, 9, 588, 2, 130], [12, 7, 637, 5, 400], [11, 6, 567, 5, 400]]


@pytest.mark.parametrize("case,floating,fric", models())
@pytest.mark.parametrize("which", [-1, 0, 1], ids=["all_columns", "merged", "regrouped"])
def test_parts_on_shipped_robots(case, floating, fric, which):
    import emul_lib

    em = emul_lib.Emul(load_topo(case), floating=floating, fric=fric)
    if which >= 0:
        red = em.reduction(which)
        if red is None:
            pytest.skip("nothing to reduce")
        em = red[0]
    for k in (0, 1):
        got = check_model(em, k)
        if got is not None and case == "walkman_apriori" and which == 1 and not fric and k == 1:
            old, new = got
            print("present cut", old[1], old[0].tolist())
            print("new cut", new[1], new[0].tolist())
            assert old[0][:, :5].astype(int).tolist() == WALKMAN_OLD
            # the slowest part of a producer WITHOUT the skip (every walked link pays its wrenches and all its entries), same coefficients
            # (a, b, c + d) = (300, 400, 6): the arm of part 2 in the present cut, as the table of the parts says
            noskip = lambda tb: 700.0 * tb[:, 0] + 6.0 * (tb[:, 2] + tb[:, 4])
            slow_old, slow_new = int(np.argmax(noskip(old[0]))), int(np.argmax(noskip(new[0])))
            assert slow_old == 2
            assert noskip(new[0]).max() < noskip(old[0]).max()
            assert new[0][slow_new, 4] < old[0][slow_old, 4], "the slowest part walks no fewer discarded entries"
            assert new[0][:, :5].astype(int).tolist() == WALKMAN_NEW


# the new cut of the same model under the instruction-count coefficients (a, b, c, d) = (300, 400, 5, 1)
WALKMAN_NEW = [[8, 8, 508, 0, 0], [10, 8, 518, 2, 130], [11, 7, 637, 4, 300], [11, 7, 637, 4, 300]]


@pytest.mark.parametrize("seed", range(16))
def test_parts_on_random_trees(seed):
    import emul_lib

    rng = np.random.default_rng(2100 + seed)
    t = random_topology(rng, 10 + 6 * (seed % 4), p_fixed=0.3, branchiness=0.5, p_prismatic=0.3 if seed % 3 == 0 else 0.0)
    if t.num_dofs == 0:
        pytest.skip("no joints")
    served = 0
    for fric in (False, True):
        em = emul_lib.Emul(t, floating=seed % 2 == 0, fric=fric)
        for cand in [em] + [r[0] for r in (em.reduction(1),) if r is not None]:
            for k in (0, 1):
                served += check_model(cand, k) is not None
    print("served", served)


@pytest.mark.parametrize("case,which,fric", [("walkman_apriori", 1, False), ("walkman_left_arm", 1, False), ("walkman_left_arm", -1, True),
                                             ("kuka_lwr4", 1, True), ("threeLinks", -1, False)])
def test_emulated_gram_from_the_destination_words(case, which, fric):
    """the emulated pass still computes the oracle's [Y | tau] Gram with weighted rows: its image holds what the destination words of the
    default producer tables say and nothing of a link without words"""
    import emul_lib

    rng = np.random.default_rng(79)
    t = load_topo(case)
    floating = case.startswith("walkman")
    om = OracleModel(t, floating=floating, fric=fric)
    em = emul_lib.Emul(t, floating=floating, fric=fric)
    E = np.eye(om.P)
    if which >= 0:
        em, E = em.reduction(which)
    assert parts(em, 1, 1) is not None
    S = 70
    st = random_states(t, S, rng, floating)
    sign = np.where(rng.random((S, t.num_dofs)) < 0.5, -1.0, 1.0) if fric else None
    Y = om.regressor(st, sign)
    tau = rng.standard_normal((Y.shape[0], 1))
    w = rng.random(Y.shape[0]) + 0.5
    got = em.gram64(st, tau, w, sign)
    assert got is not None
    Gr, _ = got
    Ea = np.zeros((em.cols + 1, om.P + 1))
    Ea[: em.cols, : om.P] = E
    Ea[-1, -1] = 1.0
    A = np.hstack([Y, tau]) * w[:, None]
    assert np.linalg.norm(Ea.T @ Gr @ Ea - A.T @ A) <= 1e-12 * np.linalg.norm(A.T @ A)
    assert np.array_equal(Gr, Gr.T)


def chunk_plan(nblocks, cap, num_cus, pgrid, rule):
    out = np.zeros(6, np.int64)
    rc = lib().gram64_chunk_plan(ctypes.c_long(nblocks), ctypes.c_long(cap), ctypes.c_long(num_cus), ctypes.c_long(pgrid), int(rule),
                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_long)))
    assert rc == 0, rc
    return dict(zip(("chb", "last_cap", "chunks", "gram_rounds", "prod_rounds", "largest"), (int(x) for x in out)))


# cap (blocks) / Gram grid / producer grid: the bench's model on 256 CUs (3 GB of 1.1 MB blocks, two producer workgroups per CU), a model
# of depth > 10 (one producer workgroup per CU), a smaller chip with a tight cap
GRIDS = [(2934, 256, 512), (2934, 256, 256), (700, 120, 240)]


@pytest.mark.parametrize("nblocks", [15625, 1954, 7813])
@pytest.mark.parametrize("cap,num_cus,pgrid", GRIDS)
def test_chunk_sizes_by_both_grids(nblocks, cap, num_cus, pgrid):
    if nblocks <= cap:
        assert lib().gram64_chunk_plan(ctypes.c_long(nblocks), ctypes.c_long(cap), ctypes.c_long(num_cus), ctypes.c_long(pgrid), 1, None) == -1
        return  # (a call that fits one chunk is one chunk: the rule is not asked)
    old, new = chunk_plan(nblocks, cap, num_cus, pgrid, 0), chunk_plan(nblocks, cap, num_cus, pgrid, 1)
    print(nblocks, cap, num_cus, pgrid, "present", old, "new", new)
    floor = -(-nblocks // num_cus)
    assert old["chb"] == cap // num_cus * num_cus and old["last_cap"] == old["chb"]  # today's rule
    assert new["gram_rounds"] <= old["gram_rounds"]
    if old["gram_rounds"] == floor:
        assert new["gram_rounds"] == floor
    assert new["gram_rounds"] >= floor
    assert new["prod_rounds"] <= old["prod_rounds"]
    assert new["largest"] <= cap and old["largest"] <= cap
    assert new["chb"] % num_cus == 0
    if (nblocks, cap, num_cus, pgrid) == (15625, 2934, 256, 512):  # the bench step: 5 x 2560 + 2825 instead of 5 x 2816 + 1545
        assert (old["chunks"], old["gram_rounds"], old["prod_rounds"]) == (6, 62, 34)
        assert (new["chb"], new["chunks"], new["gram_rounds"], new["prod_rounds"], new["largest"]) == (2560, 6, 62, 31, 2825)
