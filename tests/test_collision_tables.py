"""csrc/fbr_collision_tables.h (g++, tests/emul/collision_tables_emul.cpp): the step sort, the slot numbers and the gradient table that
fbr_model_set_capsules, fbr_model_set_boxes and fbr_model_set_hulls share, against a few lines of NumPy restating them; the packing of a
set's arrays into one allocation; the classes of a hull set's pairs and the stencil tables of its staged gradient calls, through the
emulation and through a stand-alone program under the sanitizers (tests/emul/collision_tables_sanitize.cpp)."""
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
        deps = [_SRC, os.path.join(ROOT, "include", "fbr.h")] + [os.path.join(_CSRC, h) for h in (
            "fbr_collision_tables.h", "fbr_capsule_grad.h", "fbr_capsule.h", "fbr_math.h", "fbr_kinid.h", "fbr_program.h", "fbr_mesh_grad.h", "fbr_mesh.h",
            "fbr_hull_grad.h", "fbr_hull.h", "fbr_box_grad.h", "fbr_box.h")]
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


# ---- the hull set: classes of its pairs and stencil tables (fbr_hull_pair_classes, fbr_stencil_table) ------------------------------------------
SMALL, BIG, MESH = 0, 1, 2


def hull_cases(topo):
    """name -> (link, vertices, triangles of every hull -- None: no mesh table --, pairs).  The hulls: 0 small on link 0, 1 of exactly 128
    vertices (small) on the last link, 2 of 129 (big) on link 1, 3 meshed on the last link, 4 a meshed world hull, 5 a big world hull, 6 small
    on link 1, 7 meshed on link 0."""
    L = topo.num_links
    link = np.array([0, L - 1, 1, L - 1, -1, -1, 1, 0], np.int32)
    nv = np.array([8, 128, 129, 16, 8, 200, 4, 12], np.int32)
    nt = np.array([0, 0, 0, 30, 12, 0, 0, 7], np.int32)
    mixed = [(3, 1),  # the mesh on the first member
             (0, 1),  # small: 128 vertices are not big
             (1, 2),  # big by one vertex
             (0, 3),  # the mesh on the second member (swap): its first hull ties with column 0, and sorts behind it
             (7, 3),  # both meshed: the caller's order, sorted by 7
             (6, 0), (5, 0),  # small; a big world hull
             (1, 4), (4, 6),  # a meshed world hull, second and first
             (3, 7),  # both meshed, the other way round
             (3, 2), (2, 7),  # a mesh and a big hull: MESH
             (6, 3), (3, 0)]  # ties on hull 3 in reversed column order further down
    return {
        "no pair": (link, nv, nt, []),
        "all small": (link, nv, nt, [(0, 1), (1, 6), (6, 0), (1, 0)]),
        "all big": (link, nv, nt, [(2, 0), (1, 2), (5, 0), (6, 5), (2, 5)]),
        "all mesh": (link, nv, nt, [(3, 0), (0, 3), (3, 7), (7, 3), (4, 1), (1, 4), (2, 3), (5, 7)]),
        "mixed": (link, nv, nt, mixed),
        "mixed, no mesh table": (link, nv, None, mixed),
    }


def restated_classes(nv, nt, pairs):
    """class -> (columns, pair list, swap) in a few lines of NumPy"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    meshed = (np.zeros_like(nv) if nt is None else nt)[pairs] > 0
    cls = np.where(meshed.any(1), MESH, np.where((nv[pairs] > 128).any(1), BIG, SMALL))
    out = {}
    for c in (SMALL, BIG, MESH):
        cols = np.flatnonzero(cls == c)
        swap = ~meshed[cols, 0] if c == MESH else np.zeros(len(cols), bool)
        lst = np.where(swap[:, None], pairs[cols][:, ::-1], pairs[cols])
        order = np.argsort(lst[:, 0], kind="stable") if c == MESH else np.arange(len(cols))
        out[c] = (cols[order], lst[order], swap[order].astype(np.int64))
    return out


def restated_stencil(topo, steplink, link, pairs, cols, cmode):
    """sbeg | spair | sjoint, the largest S_k: per pair the centre, then twice every joint above one member only -- or above both, for a
    revolute joint with the offsets in the world's axes (cmode 0) -- in walk order, up to the later of the two members' steps"""
    stepof = np.zeros(topo.num_links, np.int64)
    stepof[steplink] = np.arange(len(steplink))

    def above(l):
        s = set()
        while l >= 0:
            s.add(l)
            l = topo.parent[l]
        return s

    sbeg, spair, sjoint = [0], [], []
    for i, k in enumerate(cols):
        la, lb = (link[h] for h in pairs[k])
        A, B = above(la), above(lb)
        kend = max(stepof[la] if la >= 0 else -1, stepof[lb] if lb >= 0 else -1) + 1
        joints = [-1]
        for l in steplink[:kend]:
            mk = (l in A) + 2 * (l in B)
            jt = 0 if topo.parent[l] < 0 else topo.joint_type[l]
            if mk and jt != 0 and topo.dof_index[l] >= 0 and (mk != 3 or (cmode == 0 and jt == 1)):
                joints += [topo.dof_index[l]] * 2
        sbeg.append(sbeg[-1] + len(joints))
        spair += [i] * len(joints)
        sjoint += joints
    return np.array(sbeg + spair + sjoint, np.int64), int(np.diff(sbeg).max()) if len(cols) else 0


def library_classes(nv, nt, pairs):
    i = lambda a: a.ctypes.data_as(_ip)  # noqa: E731
    vbeg = np.concatenate([[0], np.cumsum(nv)]).astype(np.int32)
    mtab = None if nt is None else np.ascontiguousarray(np.stack([np.concatenate([[0], np.cumsum(nt)[:-1]]), nt], 1), np.int32)
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1)
    P = len(pr) // 2
    counts, col, lst, swap = np.full(3, -9, np.int32), np.full(P, -9, np.int32), np.full(2 * P, -9, np.int32), np.full(P, -9, np.int32)
    emul().hull_pair_classes(len(nv), i(vbeg), None if mtab is None else i(mtab), P, i(pr), i(counts), i(col), i(lst), i(swap))
    assert counts.sum() == P
    edge = np.concatenate([[0], np.cumsum(counts)])
    assert (swap[:edge[MESH]] == -1).all() and (swap[edge[MESH]:] >= 0).all()  # (only a mesh pair has a flag)
    swap[:edge[MESH]] = 0
    return {c: (col[edge[c]:edge[c + 1]], lst.reshape(-1, 2)[edge[c]:edge[c + 1]], swap[edge[c]:edge[c + 1]]) for c in (SMALL, BIG, MESH)}


def library_stencil(topo, link, pairs, cols, cmode):
    c = lambda a, t=np.float64: np.ascontiguousarray(a, dtype=t)  # noqa: E731
    i = lambda a: a.ctypes.data_as(_ip)  # noqa: E731
    d = lambda a: a.ctypes.data_as(_dp)  # noqa: E731
    parent, dof, jt = c(topo.parent, np.int32), c(topo.dof_index, np.int32), c(topo.joint_type, np.int32)
    rR, rp, ax = c(topo.rest_R).reshape(-1), c(topo.rest_p).reshape(-1), c(topo.axis).reshape(-1)
    pr, cl = c(pairs, np.int32).reshape(-1), c(cols, np.int32)
    cap = 1 + len(cl) * (3 + 4 * topo.num_dofs)
    tab, counts, direct = np.full(cap, -9, np.int32), np.full(3, -9, np.int32), np.full(max(len(cl), 1), -9, np.int32)
    size = emul().stencil_table(topo.num_links, topo.num_dofs, i(parent), i(dof), d(rR), d(rp), d(ax), i(jt), i(c(link, np.int32)), i(pr), len(cl), i(cl),
                                cmode, cap, i(tab), i(counts), i(direct))
    assert size > 0
    return tab[:size], counts, direct[:len(cl)]


def check_classes(got, ref, nv, nt, pairs):
    for c in (SMALL, BIG, MESH):
        for g, r, what in zip(got[c], ref[c], ("columns", "pair list", "swap")):
            assert np.array_equal(np.asarray(g).reshape(np.shape(r)), r), (c, what)
    cols, lst, swap = ref[MESH]
    # what the classes say: every column once; a mesh pair has its meshed hull first and is swapped only when the caller's first has none;
    # its list is sorted by that hull and, among equal hulls, by the column
    assert sorted(np.concatenate([ref[c][0] for c in (SMALL, BIG, MESH)])) == list(range(len(pairs)))
    if len(cols):
        assert (nt[lst[:, 0]] > 0).all() and all(swap[j] == (nt[pairs[k][0]] == 0) for j, k in enumerate(cols))
        assert all((lst[j, 0], cols[j]) < (lst[j + 1, 0], cols[j + 1]) for j in range(len(cols) - 1))
    assert all(nv[list(pairs[k])].max() <= 128 for k in ref[SMALL][0]) and all(nv[list(pairs[k])].max() > 128 for k in ref[BIG][0])


def check_stencil(tab, npairs, nitems, smax, ref, ref_smax, ncols):
    assert (npairs, nitems, smax) == (ncols, (len(ref) - ncols - 1) // 2, ref_smax)
    assert np.array_equal(tab, ref)
    sbeg, sjoint = tab[:ncols + 1], tab[ncols + 1 + nitems:]
    for j in range(ncols):  # S_k = 1 + 2 J_k: the centre, then every joint twice
        s = sjoint[sbeg[j]:sbeg[j + 1]]
        assert len(s) % 2 == 1 and s[0] == -1 and np.array_equal(s[1::2], s[2::2]) and (s[1:] >= 0).all()


@pytest.mark.parametrize("robot", ["threeLinks", "walkman_left_arm"])
def test_hull_pair_classes_and_stencil_tables(robot):
    topo = load_topo(robot)
    steplink = library_tables(topo, np.zeros(1, np.int32), np.zeros((0, 2), np.int32))["steplink"]
    seen = set()
    for name, (link, nv, nt, pairs) in hull_cases(topo).items():
        ref = restated_classes(nv, nt, pairs)
        check_classes(library_classes(nv, nt, pairs), ref, nv, np.zeros_like(nv) if nt is None else nt, pairs)
        seen.add(tuple(len(ref[c][0]) > 0 for c in (SMALL, BIG, MESH)))
        for cmode in (0, 1):
            for cols in [ref[c][0] for c in (SMALL, BIG, MESH)] + [np.arange(len(pairs))]:
                tab, counts, direct = library_stencil(topo, link, pairs, cols, cmode)
                want, smax = restated_stencil(topo, steplink, link, pairs, cols, cmode)
                check_stencil(tab, *counts, want, smax, len(cols))
                assert np.array_equal(np.diff(tab[:len(cols) + 1]), direct), name  # fbr_meshgrad_slots, pair by pair
    assert {(False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True), (True, True, False)} <= seen
    mixed = restated_classes(*hull_cases(topo)["mixed"][1:])
    assert list(mixed[MESH][0]) == [0, 3, 9, 10, 12, 13, 7, 8, 4, 11] and list(mixed[MESH][2]) == [0, 1, 0, 0, 1, 0, 1, 0, 0, 1]
    assert list(mixed[SMALL][0]) == [1, 5] and list(mixed[BIG][0]) == [2, 6]


@pytest.mark.parametrize("robot", ["threeLinks", "walkman_left_arm"])
def test_classes_and_stencils_under_the_sanitizers(robot, tmp_path):
    """tests/emul/collision_tables_sanitize.cpp, a program of its own, built with -fsanitize=address,undefined and run here on the CPU on the
    same cases, its output held to the same restatement"""
    exe = str(tmp_path / "collision_tables_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(_HERE, "emul", "collision_tables_sanitize.cpp")])
    topo = load_topo(robot)
    steplink = library_tables(topo, np.zeros(1, np.int32), np.zeros((0, 2), np.int32))["steplink"]
    cases = hull_cases(topo)
    words = [topo.num_links, topo.num_dofs, *topo.parent, *topo.dof_index, *topo.joint_type]
    words += [repr(float(v)) for a in (topo.rest_R, topo.rest_p, topo.axis) for v in np.asarray(a, np.float64).reshape(-1)]
    words.append(len(cases))
    for link, nv, nt, pairs in cases.values():
        words += [len(nv), *link, 0, *np.cumsum(nv), int(nt is not None)]
        if nt is not None:
            words += list(np.stack([np.concatenate([[0], np.cumsum(nt)[:-1]]), nt], 1).reshape(-1))
        words += [len(pairs), *[h for p in pairs for h in p]]
    run = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.endswith("ok\n") and not run.stderr, (run.stdout[-400:], run.stderr)
    lines = iter([np.array(ln.split(), np.int64) for ln in run.stdout.split("\n")[:-2]])
    for link, nv, nt, pairs in cases.values():
        counts = next(lines)
        got = {}
        for c in (SMALL, BIG, MESH):
            got[c] = [next(lines), next(lines).reshape(-1, 2), np.zeros(counts[c], np.int64)]
        got[MESH][2] = next(lines)
        ref = restated_classes(nv, nt, pairs)
        check_classes(got, ref, nv, np.zeros_like(nv) if nt is None else nt, pairs)
        for cmode in (0, 1):
            for cols in [ref[c][0] for c in (SMALL, BIG, MESH)] + [np.arange(len(pairs))]:
                head, tab = next(lines), next(lines)
                want, smax = restated_stencil(topo, steplink, link, pairs, cols, cmode)
                check_stencil(tab, *head, want, smax, len(cols))
    assert next(lines, None) is None
