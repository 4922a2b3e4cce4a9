"""csrc/fbr_collision_tables.h (g++, tests/emul/collision_tables_emul.cpp): the step sort, the slot numbers and the gradient table that
fbr_model_set_capsules, fbr_model_set_boxes and fbr_model_set_hulls share, against a few lines of NumPy restating them; the packing of a
set's arrays into one allocation."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from common import ROOT, load_topo

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "collision_tables_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libcollision_tables_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lib = None


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC] + [os.path.join(_CSRC, h) for h in ("fbr_collision_tables.h", "fbr_capsule_grad.h", "fbr_capsule.h", "fbr_math.h", "fbr_kinid.h",
                                                          "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
        _lib.collision_blob.restype = ctypes.c_long
    return _lib


def library_tables(topo, link, pairs):
    c = lambda a, t=np.float64: np.ascontiguousarray(a, dtype=t)  # noqa: E731
    i = lambda a: a.ctypes.data_as(_ip)  # noqa: E731
    d = lambda a: a.ctypes.data_as(_dp)  # noqa: E731
    L, nmem, P = topo.num_links, len(link), len(pairs)
    parent, dof, jt = c(topo.parent, np.int32), c(topo.dof_index, np.int32), c(topo.joint_type, np.int32)
    rR, rp, ax = c(topo.rest_R).reshape(-1), c(topo.rest_p).reshape(-1), c(topo.axis).reshape(-1)
    link, pr = c(link, np.int32), c(pairs, np.int32).reshape(-1)
    steplink, stepof, beg = np.full(L, -9, np.int32), np.full(L, -9, np.int32), np.full(L + 1, -9, np.int32)
    code, slot, ids = np.full(nmem, -9, np.int32), np.full(nmem, -9, np.int32), np.full(max(nmem, 1), -9, np.int32)
    counts, gt = np.zeros(3, np.int32), np.full(4 * max(P, 1) + L * ((L + 31) // 32), -9, np.int32)
    ns = emul().collision_tables(L, topo.num_dofs, i(parent), i(dof), d(rR), d(rp), d(ax), i(jt), nmem, i(link), P, i(pr), i(steplink), i(stepof),
                                 i(beg), i(code), i(slot), i(ids), i(counts), i(gt))
    assert ns > 0
    nrob, nworld, W = (int(v) for v in counts)
    return dict(nsteps=ns, steplink=steplink[:ns], stepof=stepof, beg=beg[:ns + 1], code=code, slot=slot, id=ids[:max(nrob, 1)], nrob=nrob,
                nworld=nworld, W=W, gt=gt[:4 * max(P, 1) + ns * W])


def restated_tables(topo, steplink, link, pairs):
    """the same tables from the order in which the program walks the links"""
    link, ns = np.asarray(link), len(steplink)
    stepof = np.zeros(topo.num_links, np.int64)
    stepof[steplink] = np.arange(ns)
    rob, wld = np.flatnonzero(link >= 0), np.flatnonzero(link < 0)
    code = np.zeros(len(link), np.int64)
    code[rob], code[wld] = np.arange(len(rob)), -1 - np.arange(len(wld))
    order = rob[np.argsort(stepof[link[rob]], kind="stable")]  # robot members by the step of their link, the caller's order within a link
    slot = np.full(len(link), -1)
    slot[order] = np.arange(len(order))
    beg = np.searchsorted(stepof[link[order]], np.arange(ns + 1))
    ids = code[order] if len(order) else np.zeros(1, np.int64)
    W = (ns + 31) // 32
    anc = np.zeros((ns, W), np.uint32)
    for k in range(ns):
        l = steplink[k]
        while l >= 0:
            anc[k, stepof[l] >> 5] |= np.uint32(1 << (stepof[l] & 31))
            l = topo.parent[l]
    rec = np.zeros((max(len(pairs), 1), 4), np.int64)
    for k, (a, b) in enumerate(pairs):
        rec[k] = [-1 if link[a] < 0 else stepof[link[a]], -1 if link[b] < 0 else stepof[link[b]], -1 - code[a] if link[a] < 0 else slot[a],
                  -1 - code[b] if link[b] < 0 else slot[b]]
    return dict(stepof=stepof, code=code, slot=slot, beg=beg, id=ids, W=W, gt=np.concatenate([rec.reshape(-1), anc.view(np.int32).reshape(-1)]))


def members(topo):
    """(link of every member, pairs): a world member first and one last in the caller's order, two members on the last link, none on link 1,
    the links in between in descending order; pairs (robot, robot), (world, robot), (robot, world) and the two members of one link"""
    L = topo.num_links
    link = [-1, L - 1, 0, L - 1] + list(range(L - 2, 1, -1)) + [-1]
    last = len(link) - 1
    pairs = [(1, 2), (0, 1), (2, last), (3, 1), (last, 3), (2, 3)]
    if L > 3:
        pairs += [(4, 1), (0, 4), (last - 1, last)]
    return np.array(link, np.int32), np.array(pairs, np.int32)


@pytest.mark.parametrize("robot", ["threeLinks", "walkman_left_arm"])
def test_sort_slots_and_gradient_table(robot):
    topo = load_topo(robot)
    link, pairs = members(topo)
    assert 1 not in link and (link == topo.num_links - 1).sum() == 2 and link[0] < 0 and link[-1] < 0
    got = library_tables(topo, link, pairs)
    # the program walks every link once, parents first
    assert sorted(got["steplink"]) == list(range(topo.num_links))
    assert all(topo.parent[l] < 0 or got["stepof"][topo.parent[l]] < got["stepof"][l] for l in range(topo.num_links))
    ref = restated_tables(topo, got["steplink"], link, pairs)
    assert got["nrob"] == (link >= 0).sum() and got["nworld"] == 2 and got["W"] == ref["W"]
    for key in ("stepof", "code", "slot", "beg", "id", "gt"):
        assert np.array_equal(got[key], ref[key]), key
    # what the tables say: link 1 has no slot, the two members of the last link sit side by side in the caller's order, the world
    # members carry -1 and their number
    k1 = got["stepof"][1]
    assert got["beg"][k1] == got["beg"][k1 + 1]
    assert got["slot"][3] == got["slot"][1] + 1
    rec = got["gt"][:4 * len(pairs)].reshape(-1, 4)
    assert list(rec[1, [0, 2]]) == [-1, 0] and list(rec[2, [1, 3]]) == [-1, 1] and rec[3, 0] == rec[3, 1]


def test_capsule_sets_have_no_world_members():
    """every member on a link: the code of a member is its number, id maps a slot back to the caller's index (DevCapsules.capid)"""
    topo = load_topo("walkman_left_arm")
    link = np.array([3, 0, 3, 2, 0], np.int32)
    got = library_tables(topo, link, np.array([(0, 1), (4, 2)], np.int32))
    assert got["nworld"] == 0 and np.array_equal(got["code"], np.arange(5))
    assert np.array_equal(got["id"][got["slot"]], np.arange(5))
    assert np.array_equal(got["stepof"][link[got["id"]]], np.sort(got["stepof"][link], kind="stable"))


@pytest.mark.parametrize("nd,ni,np_", [(3, 4, 2), (3, 5, 2), (0, 1, 1), (7, 0, 3)])
def test_blob_layout(nd, ni, np_):
    """doubles | ints | (padding to 8 bytes) pairs: every array at its alignment, nothing else in between, padding zeroed"""
    off = (ctypes.c_long * 3)()
    buf = np.full(8 * (nd + ni + 2 * np_ + 1), 0x55, np.uint8)
    size = emul().collision_blob(nd, ni, np_, off, buf.ctypes.data_as(ctypes.c_char_p))
    o_d, o_i, o_p = list(off)
    assert o_d == 0 and o_i == 8 * nd and o_p == (o_i + 4 * ni + 7) // 8 * 8 and size == o_p + 8 * np_
    raw = buf[:size].tobytes()
    assert np.array_equal(np.frombuffer(raw, np.float64, nd, o_d), 1.0 + np.arange(nd))
    assert np.array_equal(np.frombuffer(raw, np.int32, ni, o_i), 100 + np.arange(ni))
    assert np.array_equal(np.frombuffer(raw, np.int32, 2 * np_, o_p), 1000 + np.arange(2 * np_))
    assert not any(raw[o_i + 4 * ni:o_p])
