"""fbr_candidate_hull_distances / Engine.candidate_hull_distances on the device against the g++ emulation of the same text
(tests/emul/hull_emul.cpp) and the Qhull restatement (tests/hull_restatement.py).

The bar of a (candidate, pair) is, at the restatement's winning sample, the larger of 10 x the largest deviation the emulation shows
against the restatement on the same inputs, and 32 eps x the pair's scale |cB - cA| + diam A + diam B.  Every minimum has to lie within
the bar of the emulation's, every index has to be the restatement's argmin: the committed seeds keep the runner-up more than 100 bars above
the minimum for every pair, and both signs occur among the minima -- asserted on the CPU before the device is asked.  C = 3 candidates of
T = 200 samples at step 3: 67 checked samples a candidate, a full block of 64 and one of 3; the pairs fill more than one batch of 16 and
are no multiple of it.  The references are computed once a case and shared by its tests.

Seen on an MI355X over all cases of this file: |device - emulation| <= 2.2e-16, at most 0.014 of the bar (bars 6.8e-15 to 1.0e-14; the
emulation's deviation from the restatement on the same inputs 3.3e-16 to 1.0e-15), |device - restatement| <= 4.9e-16; the box kernel and
the hull kernel on the same boxes differ by 1.2e-16 at most ("Convex-hull collision distances")."""
import functools
import os

import numpy as np
import pytest

import box_restatement as br
import hull_restatement as hr
from common import GOLDEN, load_topo, random_states
from test_gpu_boxes import _dev, _engine, _host, _moving_joints, three_links_case
from test_gpu_boxes import case_pairs as box_case_pairs
from test_hulls import EPS, as_tuples, emul_eval, left_arm_hulls

pytestmark = pytest.mark.gpu
BATCH = 16  # FBR_HULL_BATCH
C, T, STEP = 3, 200, 3


def reference(topo, floating, hulls, pairs, st, bp, mode):
    """(val, idx, bar, emulation's minima, emulation - restatement) (C, P) the device has to meet, after the assertions on the CPU's side"""
    assert len(pairs) > BATCH and len(pairs) % BATCH != 0
    rows = [c * T + i for c in range(C) for i in range(0, T, STEP)]
    assert len(rows) == C * 67
    tup = as_tuples(topo, hulls)
    R, cen = hr.hull_world(topo, tup, st["q"], floating, st.get("rpy"), bp, mode)
    want, scale = hr.pair_distances(R, cen, tup, pairs, rows)
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
    assert np.all(runner - val > 100.0 * cbar), "a runner-up lies within 100 bars of the minimum: change the seed"
    assert (val > 0).any() and (val <= 0).any(), "both signs among the minima"
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
    return topo, hl, pairs, st, bp, reference(topo, True, hl, pairs, st, bp, mode)


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
    return topo, boxes, hl, pairs, st, reference(topo, False, hl, pairs, st, None, mode)


def run(eng, hulls, pairs, st, bp, mode, ref, device, why):
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
