"""fbr_candidate_hull_distances / Engine.candidate_hull_distances on the device against the g++ emulation of the same text
(tests/emul/hull_emul.cpp) and the Qhull restatement (tests/hull_restatement.py).

The bar of a (candidate, pair) is, at the restatement's winning sample, the larger of 10 x the largest deviation the emulation shows
against the restatement on the same inputs, and 32 eps x the pair's scale |cB - cA| + diam A + diam B.  Every minimum has to lie within
the bar of the emulation's, every index has to be the restatement's argmin: the committed seeds keep the runner-up more than 100 bars above
the minimum for every pair, and both signs occur among the minima -- asserted on the CPU before the device is asked.  C = 3 candidates of
T = 200 samples at step 3: 67 checked samples a candidate, a full block of 64 and one of 3; the pairs fill more than one batch of 16 and
are no multiple of it.  The references are computed once a case and shared by its tests.

The cases on the shapes of tests/hull_shapes.py hold the device to the same bar (reference(): a tenth of the minima at least on either
side of 0) at C = 2 or 4, T = 67, step 1.  Random trees with fixed and prismatic joints, fixed and floating base: hulls of every kind from
4 to 128 vertices, two on some links and none on others, world hulls in between, the hull list and the pair list shuffled, world hulls
first in some pairs -- host and device states, one block a launch and each candidate alone give the same bits; the pairs in another order
give the same columns bit for bit, swapped pairs the same winners within the bar, the hull list in another order the same bits.  A gantry
of two prismatic joints with exact poses: hulls that touch at a vertex, an edge or a face at gaps of 1e-9, 0, -1e-9 and -1e-3, reached in
one lane of the wave, which wins.

Seen on an MI355X over the left arm and threeLinks: |device - emulation| <= 2.2e-16, at most 0.014 of the bar (bars 6.8e-15 to 1.0e-14;
the emulation's deviation from the restatement on the same inputs 3.3e-16 to 1.0e-15), |device - restatement| <= 4.9e-16; the box kernel
and the hull kernel on the same boxes differ by 1.2e-16 at most.  Over the random trees, reordered or not: |device - emulation| <=
1.8e-15, 0.029 of the bar at worst (bars 3.1e-14 and 4.2e-14), 15 GJK iterations at most.  Over the gantry: the device returns the
emulation's bits with the carriage turned by pi and by pi / 2, and is within 4.4e-16 = 0.012 of the bar (8.9e-15) with pi / 4, the
contact pairs alone within 0.0082; 12 iterations at most ("Convex-hull collision distances")."""
import functools
import os
import time

import numpy as np
import pytest

import box_restatement as br
import hull_restatement as hr
import hull_shapes as hs
from common import GOLDEN, load_topo, random_states, random_topology
from test_gpu_boxes import _dev, _engine, _host, _moving_joints, three_links_case
from test_gpu_boxes import case_pairs as box_case_pairs
from test_hulls import EPS, as_tuples, emul_eval, left_arm_hulls

pytestmark = pytest.mark.gpu
BATCH = 16  # FBR_HULL_BATCH
C, T, STEP = 3, 200, 3


def reference(topo, floating, hulls, pairs, st, bp, mode, C, T, STEP, share=0.0):
    """(val, idx, bar, emulation's minima, emulation - restatement) (C, P) the device has to meet, after the assertions on the CPU's side;
    ``share``: the part of the minima that has to lie on either side of 0 at least (one of each in any case)"""
    assert len(pairs) > BATCH and len(pairs) % BATCH != 0
    rows = [c * T + i for c in range(C) for i in range(0, T, STEP)]
    assert len(rows) == C * 67
    tup = as_tuples(topo, hulls)
    R, cen = hr.hull_world(topo, tup, st["q"], floating, st.get("rpy"), bp, mode)
    t0 = time.process_time()
    want, scale = hr.pair_distances(R, cen, tup, pairs, rows)
    t0 = time.process_time() - t0
    _, emu, iters = emul_eval(topo, floating, hulls, pairs, st["q"], st.get("rpy") if floating else None, bp if floating else None, mode)
    assert (iters % 1000).max() * 2 <= 64
    fin = np.isfinite(want)
    dev = float(np.abs(emu - want)[fin].max())
    bar = np.maximum(10.0 * dev, 32.0 * EPS * scale)
    val, idx = hr.candidate_minimum(np.where(fin, want, np.inf), C, STEP)
    eval_, eidx = hr.candidate_minimum(emu, C, STEP)
    w3 = np.where(fin, want, np.inf).reshape(C, T, -1)[:, ::STEP]
    cbar = np.take_along_axis(bar.reshape(C, T, -1)[:, ::STEP], (idx // STEP)[:, None, :], axis=1)[:, 0]
    runner = np.sort(w3, axis=1)[:, 1]
    print(f"hull reference: {len(hulls)} hulls, {len(pairs)} pairs, {len(rows)} samples; the restatement took {t0:.1f} s; most GJK iterations "
          f"{(iters % 1000).max()}; smallest (runner-up - minimum) / bar {((runner - val) / cbar).min():.3g}; minima <= 0: {(val <= 0).sum()} of {val.size}")
    assert np.all(runner - val > 100.0 * cbar), "a runner-up lies within 100 bars of the minimum: change the seed"
    assert (val > 0).any() and (val <= 0).any(), "both signs among the minima"
    assert (val > 0).mean() >= share and (val <= 0).mean() >= share, "the share of either sign among the minima"
    assert np.array_equal(eidx, idx) and np.all(np.abs(eval_ - val) <= cbar)
    return val, idx, cbar, eval_, dev


@functools.lru_cache(maxsize=None)
def left_arm_case(placement, mode):
    """the floating left arm with its nine mesh hulls (offsets a few centimetres off the link origins, so that the two placements differ) and
    the four boxes of world_walkman_suspended.urdf as hulls"""
    from flobaroid_amd.collision import world_hulls_from_urdf

    rng = np.random.default_rng(11)
    topo, (hulls, _) = left_arm_hulls()
    wh = world_hulls_from_urdf(os.path.join(GOLDEN, "urdf", "world_walkman_suspended.urdf"), placement)
    for h in hulls.values():
        h.offset = rng.uniform(-0.03, 0.03, 3)
    hl = [hulls[n] for n in topo.link_names if n in hulls] + list(wh.values())
    st = random_states(topo, C * T, rng, True, use_limits=True)
    st["rpy"] = rng.uniform(-0.6, 0.6, (C * T, 3))
    bp = wh["crane_tip"].offset + rng.standard_normal((C * T, 3)) * 0.15
    names = list(topo.link_names)
    link = [names.index(h.link_name) if h.link_name else -1 for h in hl]
    rob, wld = [i for i, l in enumerate(link) if l >= 0], [i for i, l in enumerate(link) if l < 0]
    pairs = []
    for i in rob:  # robot pairs three moving joints apart at least (an arm's neighbours overlap all the time), the crane's arm and tip in between
        mine = [(i, j) for j in rob if j > i and _moving_joints(topo, link[i], link[j]) >= 3]
        wp = [(i, w) for w in wld[2:]]
        for k in range(max(len(mine), len(wp))):
            pairs += mine[k:k + 1] + wp[k:k + 1]
    pairs = np.array(pairs, dtype=np.int32).reshape(-1, 2)[::2]  # (every other one: the Qhull restatement of a mesh pair takes milliseconds a sample)
    if len(pairs) % BATCH == 0:
        pairs = pairs[:-1]
    return topo, hl, pairs, st, bp, reference(topo, True, hl, pairs, st, bp, mode, C, T, STEP)


@functools.lru_cache(maxsize=None)
def three_links_boxes(placement, mode):
    """threeLinks with five boxes a link over the tilted floor of world_kuka.urdf (tests/test_gpu_boxes.py), as boxes and as hulls"""
    from flobaroid_amd.collision import Box, hull_from_box

    rng = np.random.default_rng(7)
    topo, boxes, st = three_links_case(rng, placement, C, T, mode)
    pairs = box_case_pairs(topo, boxes, False)[::2]
    if len(pairs) % BATCH == 0:
        pairs = pairs[:-1]
    hl = [hull_from_box(Box(topo.link_names[l] if l >= 0 else None, h, c, r, "floor" if l < 0 else None)) for l, h, c, r in boxes]
    return topo, boxes, hl, pairs, st, reference(topo, False, hl, pairs, st, None, mode, C, T, STEP)


def run(eng, hulls, pairs, st, bp, mode, ref, device, why, C=C, STEP=STEP):
    val, idx, bar, emu, dev = ref
    eng.set_hulls(hulls, pairs, offset_in_link_axes=mode)
    s2 = {k: st[k] for k in ("q", "rpy") if k in st}
    if device:
        import torch

        got = eng.candidate_hull_distances(_dev(s2), C, STEP, base_pos=None if bp is None else torch.from_numpy(bp).cuda())
        assert hasattr(got["dist"], "cpu")
    else:
        got = eng.candidate_hull_distances(s2, C, STEP, base_pos=bp)
    got = _host(got)
    assert got["dist"].shape == val.shape and got["idx"].dtype == np.int64
    err = np.abs(got["dist"] - emu)
    print(f"hull case {why}: max |device - emulation| = {err.max():.3e} = {(err / bar).max():.3f} bars, |device - restatement| = "
          f"{np.abs(got['dist'] - val).max():.3e} (emulation - restatement {dev:.3e}; smallest bar {bar.min():.3e}); minima <= 0: {(val <= 0).sum()} of {val.size}")
    assert np.array_equal(got["idx"], idx), why
    assert np.all(err <= bar), why
    return got


@pytest.mark.parametrize("placement,mode", [("geometric", True), ("reference", False)])
def test_left_arm_mesh_hulls_under_the_crane(placement, mode):
    topo, hl, pairs, st, bp, ref = left_arm_case(placement, mode)
    eng = _engine(topo, True)
    a = run(eng, hl, pairs, st, bp, mode, ref, False, f"left arm {placement} host")
    b = run(eng, hl, pairs, st, bp, mode, ref, True, f"left arm {placement} device")
    assert a["dist"].tobytes() == b["dist"].tobytes() and np.array_equal(a["idx"], b["idx"])


@pytest.mark.parametrize("placement,mode", [("geometric", True), ("reference", False)])
def test_three_links_box_hulls_and_the_box_kernel(placement, mode):
    topo, boxes, hl, pairs, st, ref = three_links_boxes(placement, mode)
    eng = _engine(topo, False)
    a = run(eng, hl, pairs, st, None, mode, ref, False, f"threeLinks {placement} host")
    b = run(eng, hl, pairs, st, None, mode, ref, True, f"threeLinks {placement} device")
    assert a["dist"].tobytes() == b["dist"].tobytes() and np.array_equal(a["idx"], b["idx"])
    # the same boxes through the box kernel: equal within the bar, the same winners
    eng.set_boxes(boxes, pairs, center_in_link_axes=mode)
    bx = _host(eng.candidate_box_distances({"q": st["q"]}, C, STEP))
    print(f"box kernel against hull kernel: {np.abs(bx['dist'] - a['dist']).max():.3e} = {(np.abs(bx['dist'] - a['dist']) / ref[2]).max():.3f} bars")
    assert np.array_equal(bx["idx"], a["idx"]) and np.all(np.abs(bx["dist"] - a["dist"]) <= ref[2])


def test_rules_nan_rows_no_winner_and_the_same_bits():
    topo, boxes, hl, pairs, st, ref = three_links_boxes("geometric", True)
    eng = _engine(topo, False)
    got = run(eng, hl, pairs, st, None, True, ref, True, "before the NaN rows")
    again = _host(eng.candidate_hull_distances(_dev({"q": st["q"]}), C, STEP))
    assert again["dist"].tobytes() == got["dist"].tobytes() and again["idx"].tobytes() == got["idx"].tobytes()
    # a NaN row of q never wins: knock out the winning sample of pair 0 in every candidate, another sample has to win
    q = st["q"].copy()
    for c in range(C):
        q[c * T + got["idx"][c, 0]] = np.nan
    g2 = _host(eng.candidate_hull_distances({"q": q}, C, STEP))
    assert np.all(g2["idx"][:, 0] != got["idx"][:, 0]) and np.all(g2["dist"][:, 0] > got["dist"][:, 0]) and np.all(g2["idx"] % STEP == 0)
    # a candidate of NaNs: no sample wins, 1e10 / -1; its neighbours keep their bits
    q = st["q"].copy()
    q[T:2 * T] = np.nan
    g3 = _host(eng.candidate_hull_distances({"q": q}, C, STEP))
    assert np.all(g3["dist"][1] == 1e10) and np.all(g3["idx"][1] == -1)
    assert g3["dist"][[0, 2]].tobytes() == got["dist"][[0, 2]].tobytes() and np.array_equal(g3["idx"][[0, 2]], got["idx"][[0, 2]])


def test_refused_sets_leave_the_set_in_place_and_the_sets_do_not_touch_each_other():
    from flobaroid_amd._lib import FbrError
    from flobaroid_amd.collision import Hull

    topo, boxes, hl, pairs, st, ref = three_links_boxes("geometric", True)
    eng = _engine(topo, False)
    with pytest.raises(FbrError, match="code -1"):  # no hull set
        eng.candidate_hull_distances({"q": st["q"]}, C, STEP)
    eng.set_boxes(boxes, pairs, center_in_link_axes=True)
    want_b = _host(eng.candidate_box_distances({"q": st["q"]}, C, STEP))
    want = run(eng, hl, pairs, st, None, True, ref, False, "set in place")
    w = len(hl) - 1  # the floor
    tup = lambda h, **kw: tuple(kw.get(k, v) for k, v in (("link", h.link_name), ("offset", h.offset), ("rot", h.rot), ("vertices", h.vertices),  # noqa: E731
                                                             ("planes", h.planes), ("edges", h.edges)))
    skew = hl[0].planes.copy()
    skew[0, :3] *= 1.0 + 1e-8
    out = hl[0].vertices.copy()
    out[0] *= 1.001
    same = hl[0].edges.copy()
    same[2, 3] = same[2, 2]
    t = np.linspace(0, 2 * np.pi, 65, endpoint=False)
    big = Hull(hl[0].link_name, np.concatenate([np.stack([np.cos(t), np.sin(t), np.full(65, z)], 1) for z in (-0.5, 0.5)]), np.zeros(3))
    bad = [([tup(hl[0], link=99)], []), (hl, [[0, len(hl)]]), (hl, [[1, 1]]), (hl + [hl[w]], [[w, w + 1]]),
           ([tup(hl[0], offset=np.array([0.0, np.nan, 0.0]))] + hl[1:], pairs), ([tup(hl[0], planes=skew)] + hl[1:], pairs),
           ([tup(hl[0], vertices=out)] + hl[1:], pairs), ([tup(hl[0], edges=same)] + hl[1:], pairs), ([big] + hl[1:], pairs), ([hl[0]] * 4097, pairs)]
    for h, p in bad:
        with pytest.raises(FbrError, match="code -1"):
            eng.set_hulls(h, p)
    with pytest.raises(ValueError):  # a world hull without its rotation (the binding; the library refuses rot = NULL the same way)
        eng.set_hulls(hl[:w] + [tup(hl[w], link=None, rot=None)], pairs)
    assert eng.num_hull_pairs == len(pairs)
    again = _host(eng.candidate_hull_distances({"q": st["q"]}, C, STEP))  # the set in place before the refused calls
    assert again["dist"].tobytes() == want["dist"].tobytes() and again["idx"].tobytes() == want["idx"].tobytes()
    got_b = _host(eng.candidate_box_distances({"q": st["q"]}, C, STEP))
    assert got_b["dist"].tobytes() == want_b["dist"].tobytes()
    eng.set_boxes([], [])
    again = _host(eng.candidate_hull_distances({"q": st["q"]}, C, STEP))
    assert again["dist"].tobytes() == want["dist"].tobytes()
    eng.set_hulls(hl, np.zeros((0, 2)))
    with pytest.raises(FbrError, match="code -1"):  # npairs = 0
        eng.candidate_hull_distances({"q": st["q"]}, C, STEP)
    eng.set_hulls([], [])
    with pytest.raises(FbrError, match="code -1"):  # cleared
        eng.candidate_hull_distances({"q": st["q"]}, C, STEP)
    assert np.isfinite(eng.inverse_dynamics(st, topo.x_std())).all()


# ---- random trees, hull lists in any order, the vertex cap (tests/hull_shapes.py) ----------------------------------------------------------------
TC, TT = 2, 67  # candidates and samples of the cases below, at step 1: a full block of 64 and one of 3 live lanes


@functools.lru_cache(maxsize=None)
def tree_case(seed):
    """A random tree with fixed and prismatic joints (random_tree_case of tests/test_gpu_boxes.py; odd seed: floating base and offsets in
    link axes).  Hulls of every kind of the zoo, a second hull on some links, none on others, three world hulls among the link positions,
    the list shuffled; pairs by the rules of case_pairs, shuffled, every other world pair with the world hull first, cut to 23 with one pair
    whose Minkowski difference has more than 4096 points (two 128-vertex hulls; a second one alone adds 2 .. 5 s to the Qhull restatement
    of a case, which took 3.6 s to 14 s on the CPUs it has run on)."""
    rng = np.random.default_rng(seed)
    topo = random_topology(rng, int(rng.integers(6, 12)), p_fixed=0.25, branchiness=0.5, p_prismatic=0.3)
    fl = mode = bool(seed % 2)
    st = random_states(topo, TC * TT, rng, fl)
    bp = rng.standard_normal((TC * TT, 3)) * 0.2 if fl else None
    _, p = br.link_poses(topo, st["q"], fl, st.get("rpy"), bp)
    L = topo.num_links
    links = [int(l) for l in rng.permutation(L)]
    bare, twice = links[:2], links[2:5]  # no hull; two hulls
    kinds = [k for k in hs.KINDS if k != "slab"] + ["prism128", "box", "hexprism", "cone128", "tetra", "box", "hexprism"]
    on = [l for l in range(L) if l not in bare] + twice
    hl = [hs.zoo(rng, topo.link_names[l], kinds[i % len(kinds)]) for i, l in enumerate(on)]
    for kind in ("slab", "sphere128", "tetra"):
        w = hs.zoo(rng, None, kind)
        w.offset = np.concatenate(list(p))[rng.integers(L * TC * TT)] + rng.standard_normal(3) * 0.2 - (w.rot[:, 2] * 0.8 if kind == "slab" else 0.0)
        hl.append(w)
    hl = [hl[i] for i in rng.permutation(len(hl))]
    link = [topo.link_names.index(h.link_name) if h.link_name else -1 for h in hl]
    assert {len(h.vertices) for h in hl} >= {4, 8, 12, 20, 128} and sorted(link) != link and len(set(link)) < len(link)
    stub = [(l, None, None, None) for l in link]
    pairs = [(int(a), int(b)) for a, b in box_case_pairs(topo, stub, fl)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    out, big, flip = [], 0, False
    for a, b in pairs:
        if len(hl[a].vertices) * len(hl[b].vertices) > 4096:
            if big == 1:
                continue
            big += 1
        if link[b] < 0:
            flip = not flip
            a, b = (b, a) if flip else (a, b)
        out.append((a, b))
        if len(out) == 23:
            break
    pairs = np.array(out, dtype=np.int32)
    assert len(pairs) == 23 and (np.array(link)[pairs[:, 0]] < 0).sum() >= 2 and (np.array(link)[pairs[:, 1]] < 0).sum() >= 2 and big == 1
    assert (np.diff(pairs[:, 0]) < 0).any()  # (not sorted by the first hull)
    return topo, fl, mode, hl, pairs, st, bp, reference(topo, fl, hl, pairs, st, bp, mode, TC, TT, 1, share=0.1)


def _states(st, bp, rows=slice(None)):
    return {k: st[k][rows] for k in ("q", "rpy") if k in st}, None if bp is None else bp[rows]


def _call(eng, st, bp, ncand, rows=slice(None)):
    import torch

    s2, b2 = _states(st, bp, rows)
    return _host(eng.candidate_hull_distances(_dev(s2), ncand, 1, base_pos=None if b2 is None else torch.from_numpy(np.ascontiguousarray(b2)).cuda()))


def _same(a, b):
    return a["dist"].tobytes() == b["dist"].tobytes() and a["idx"].tobytes() == b["idx"].tobytes()


def _within(got, ref, why):
    """the device's ``got`` against the reference of the case (run()'s two assertions), printed in bars"""
    val, idx, bar, emu, dev = ref
    err = np.abs(got["dist"] - emu)
    print(f"hull case {why}: max |device - emulation| = {err.max():.3e} = {(err / bar).max():.3f} bars")
    assert np.array_equal(got["idx"], idx), why
    assert np.all(err <= bar), why


@pytest.mark.parametrize("seed", [3, 4])
def test_random_trees_with_shuffled_hulls_and_pairs(seed):
    topo, fl, mode, hl, pairs, st, bp, ref = tree_case(seed)
    eng = _engine(topo, fl)
    a = run(eng, hl, pairs, st, bp, mode, ref, False, f"tree {seed} host", TC, 1)
    b = run(eng, hl, pairs, st, bp, mode, ref, True, f"tree {seed} device", TC, 1)
    assert _same(a, b)
    # one block a launch: a candidate's two blocks are folded across launches, the same bits
    eng2 = _engine(topo, fl, options={"chunk_samples": 64})
    c = run(eng2, hl, pairs, st, bp, mode, ref, True, f"tree {seed}, one block a launch", TC, 1)
    assert _same(a, c)
    # a candidate alone gives the bits of its row
    for k in range(TC):
        one = _call(eng, st, bp, 1, slice(k * TT, (k + 1) * TT))
        assert one["dist"].tobytes() == a["dist"][k:k + 1].tobytes() and one["idx"].tobytes() == a["idx"][k:k + 1].tobytes()


@pytest.mark.parametrize("seed", [3, 4])
def test_pair_order_swapped_pairs_and_hull_order(seed):
    """The host tables of fbr_model_set_hulls under reorderings of the same case.  Pairs in another order: the columns in that order, bit for
    bit.  Every pair as (b, a): the indices, and the distances within the bar (the frame of A changes, so not the bits).  The hull list in
    another order with the pairs remapped: the indices and the bar, and the bits as well -- asserted, since the emulation returns equal
    bits for the two orders (a pair's value depends on its two hulls and the sample only), which is asserted first."""
    topo, fl, mode, hl, pairs, st, bp, ref = tree_case(seed)
    rng = np.random.default_rng(100 + seed)
    eng = _engine(topo, fl)
    eng.set_hulls(hl, pairs, offset_in_link_axes=mode)
    a = _call(eng, st, bp, TC)
    _within(a, ref, f"tree {seed}")
    perm = rng.permutation(len(pairs))
    assert not np.array_equal(perm, np.arange(len(pairs)))
    eng.set_hulls(hl, pairs[perm], offset_in_link_axes=mode)
    b = _call(eng, st, bp, TC)
    assert b["dist"].tobytes() == np.ascontiguousarray(a["dist"][:, perm]).tobytes() and np.array_equal(b["idx"], a["idx"][:, perm])
    eng.set_hulls(hl, pairs[:, ::-1], offset_in_link_axes=mode)
    _within(_call(eng, st, bp, TC), ref, f"tree {seed}, every pair swapped")
    order = rng.permutation(len(hl))  # the new list: hl[order[0]], hl[order[1]], ...
    new_of = np.argsort(order)
    hl2, pairs2 = [hl[i] for i in order], new_of[pairs].astype(np.int32)
    q, rpy, bpos = st["q"], st.get("rpy") if fl else None, bp if fl else None
    assert np.array_equal(emul_eval(topo, fl, hl2, pairs2, q, rpy, bpos, mode)[1], emul_eval(topo, fl, hl, pairs, q, rpy, bpos, mode)[1])
    eng.set_hulls(hl2, pairs2, offset_in_link_axes=mode)
    d = _call(eng, st, bp, TC)
    _within(d, ref, f"tree {seed}, the hull list in another order")
    assert _same(a, d)


# ---- exact contacts on the gantry -----------------------------------------------------------------------------------------------------------------
GAPS = (1e-9, 0.0, -1e-9, -1e-3)  # one candidate each
TOUCH = (5, 40, 63, 65)          # the sample of the candidate that reaches its gap: lanes of the full block, its last lane, the block of 3
LIFT = 0.25                      # the lift at which every contact pair of a gantry case touches


@functools.lru_cache(maxsize=None)
def gantry_case(turn, mode):
    """Four columns, 1.5 m apart in x, of a hull on the bed and a hull on the carriage that touch when the lift is 0.25 and the slide 0:
    B's lowest feature straight above A's highest, by the exact rest rotation of the carriage.  "apex_down": edge on edge, apex on face,
    apex on apex, the lowest vertex of a tetrahedron on the highest of the 128-vertex sphere; "on_side": a 64-gon prism's side edge on a
    prism's cap, an octagonal prism's side edge on a face, an edge of a roof on a ridge, a cone's base vertex on a face; "quarter" (z is a
    rounded number there, the restatement says where the two are): a box's edge on a face, a roof's edge on a ridge, a cube's edge on a
    prism's cap, a tetrahedron on the sphere.  The pairs: the four contacts, every other pair of a bed hull and a carriage hull whose
    Minkowski difference has no more than 4096 points, and a tilted world box beside the columns, first or second in its four pairs;
    shuffled.  The lift of candidate c is 0.25 + GAPS[c] + a V of slopes 2^-9 and 3 x 2^-10 a sample about the sample TOUCH[c], the slide a
    ramp of slopes 2^-7 and 3 x 2^-9 through 0 there: the touching lane wins its pair, and its neighbours in the wave are 2 mm and more
    apart.  The Qhull restatement of a case took 2.4 s to 11 s on the CPUs it has run on."""
    from scipy.spatial.transform import Rotation

    from flobaroid_amd.collision import Hull

    topo = hs.turned_gantry(turn)
    R = hs.TURNS[turn]
    rng = np.random.default_rng(31)
    cube, cone, ridge_y, roof_x = hs.box([0.25, 0.25, 0.25]), hs.cone(127, 0.25, 0.5), hs.wedge(0.25, 0.5, 0.25, "y"), hs.wedge(0.25, 0.5, 0.25, "x")
    ball, shift = hs.fibonacci_sphere(128, 0.25), (0.0625, -0.03125)
    cols = {"apex_down": [(ridge_y, roof_x, shift), (cube, cone, shift), (hs.cone(15, 0.25, 0.5), cone, (0.0, 0.0)), (ball, hs.tetra(rng, 0.125), None)],
            "on_side": [(hs.prism(8, 0.25, 0.5), hs.prism(64, 0.25, 0.5), shift), (cube, hs.prism(8, 0.25, 0.5), shift), (ridge_y, roof_x, shift), (cube, cone, None)],
            "quarter": [(cube, hs.box([0.25, 0.125, 0.125]), shift), (ridge_y, roof_x, shift), (hs.prism(64, 0.25, 0.5), cube, shift),
                        (ball, hs.tetra(rng, 0.125), None)]}[turn]
    bed, car = [], []
    for k, (va, vb, xy) in enumerate(cols):
        wb = vb @ R.T
        ia, ib = int(np.argmax(va[:, 2])), int(np.argmin(wb[:, 2]))
        if xy is None:  # B's lowest vertex over A's highest (the sphere), or over the face (the cube)
            xy = (va[ia, :2] if len(va) > 8 else np.array(shift)) - wb[ib, :2]
        # the carriage's origin at the contact: (0.25, 0, 0.5 + LIFT); the bed hull of column k at (0.25 + 1.5 k, 0, 0)
        w = np.array([1.5 * k + xy[0], xy[1], (va[ia, 2] - wb[ib, 2]) - (0.5 + LIFT)])
        bed.append(Hull("bed", va, np.array([0.25 + 1.5 * k, 0.0, 0.0])))
        car.append(Hull("carriage", vb, R.T @ w if mode else w))
    wall = Hull(None, hs.box([3.0, 0.25, 0.25]), np.array([2.5, 0.625, 0.875]), Rotation.from_euler("xyz", [0.4, 0.05, 0.1]).as_matrix(), "wall")
    hl = [car[2], bed[0], wall, car[0], bed[3], bed[1], car[3], car[1], bed[2]]
    at = {id(h): i for i, h in enumerate(hl)}
    pairs = [(at[id(a)], at[id(b)]) for i, a in enumerate(bed) for j, b in enumerate(car) if i == j or len(a.vertices) * len(b.vertices) <= 4096]
    pairs += [((at[id(wall)], at[id(b)]) if k % 2 else (at[id(b)], at[id(wall)])) for k, b in enumerate(car)]
    pairs = np.array([pairs[i] for i in rng.permutation(len(pairs))], dtype=np.int32)
    q = np.zeros((len(GAPS) * TT, 2))
    for c, (gap, k0) in enumerate(zip(GAPS, TOUCH)):
        i = np.arange(TT) - k0
        q[c * TT:(c + 1) * TT, 0] = (LIFT + gap) + np.where(i < 0, -i * 2.0 ** -9, i * 3.0 * 2.0 ** -10)
        q[c * TT:(c + 1) * TT, 1] = np.where(i < 0, i * 2.0 ** -7, i * 3.0 * 2.0 ** -9)
    st = {"q": q}
    ref = reference(topo, False, hl, pairs, st, None, mode, len(GAPS), TT, 1, share=0.1)
    contact = [int(np.nonzero((pairs == (at[id(a)], at[id(b)])).all(axis=1))[0][0]) for a, b in zip(bed, car)]
    # by construction: the contact pairs win at the touching sample, apart by the gap, touching, or no deeper than the gap
    val, idx = ref[0][:, contact], ref[1][:, contact]
    assert np.all(idx == np.array(TOUCH)[:, None])
    assert np.all(np.abs(val[0] - GAPS[0]) <= 1e-14) and np.all(np.abs(val[1]) <= 64 * EPS) and np.all((val[2:] <= 0) & (val[2:] >= np.array(GAPS[2:])[:, None] - 1e-14))
    assert (ref[0] > 0).any() and (ref[0] <= 0).any()
    return topo, hl, pairs, st, ref, contact


@pytest.mark.parametrize("turn,mode", [("apex_down", True), ("on_side", False), ("quarter", True)])
def test_exact_contacts_on_the_gantry(turn, mode):
    topo, hl, pairs, st, ref, contact = gantry_case(turn, mode)
    eng = _engine(topo, False)
    a = run(eng, hl, pairs, st, None, mode, ref, False, f"gantry {turn} host", len(GAPS), 1)
    b = run(eng, hl, pairs, st, None, mode, ref, True, f"gantry {turn} device", len(GAPS), 1)
    assert _same(a, b)
    err = (np.abs(a["dist"] - ref[3]) / ref[2])[:, contact]
    print(f"gantry {turn}: the contact pairs alone, |device - emulation| in bars by gap {dict(zip(GAPS, err.max(axis=1).round(4).tolist()))}")
    for k in range(len(GAPS)):
        one = _call(eng, st, None, 1, slice(k * TT, (k + 1) * TT))
        assert one["dist"].tobytes() == a["dist"][k:k + 1].tobytes() and one["idx"].tobytes() == a["idx"][k:k + 1].tobytes()
