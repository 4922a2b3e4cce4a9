"""fbr_candidate_box_distances / Engine.candidate_box_distances on the device against the NumPy restatement (tests/box_restatement.py).

The bar of a (candidate, pair) is, at the restatement's winning sample, the larger of 10 x the largest deviation the g++ emulation of the
same text (tests/emul/box_emul.cpp) shows against the restatement on the same inputs, and 32 eps x the pair's scale |cB - cA| + |hA| + |hB|.
The index has to be the restatement's argmin for every (candidate, pair): the committed seeds keep the runner-up more than 100 bars above
the minimum everywhere, which is asserted -- like the shares of overlapping and separated evaluations (10 % each at least) -- on the
restatement's side before the device is asked.  Nothing is left out.  Pairs of links with fewer than two moving joints between them (the
reference's neighbours) and the fixed base against the world are not part of the cases: their overlap ties by construction.

Largest |device - restatement| seen on an MI355X over all cases of this file: 1.9e-15 (random tree 4), at most 0.026 of the bar; the
emulation's deviation on the same inputs was 2.8e-16 (threeLinks) to 2.9e-14 (the left arm), so the bars ranged from 4.2e-15 to 2.9e-13
("Box collision distances")."""
import os

import numpy as np
import pytest

import box_restatement as br
from common import GOLDEN, load_topo, random_states, random_topology
from test_boxes import EPS, emul_eval, synthetic_boxes, world_boxes_near

pytestmark = pytest.mark.gpu
BATCH = 16  # FBR_BOX_BATCH


def _engine(topo, floating, options=None):
    from flobaroid_amd._lib import Engine

    return Engine(topo, floating=floating, options=options)


def _dev(st):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in st.items()}


def _host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _moving_joints(topo, la, lb):
    """number of revolute / prismatic joints on the tree path between link la and link lb (-1: the base's parent, i.e. the world)"""
    def chain(l):
        out = []
        while l >= 0:
            out.append(l)
            l = topo.parent[l]
        return out

    ca, cb = chain(la), (chain(lb) if lb >= 0 else [])
    common = set(ca) & set(cb)
    path = [l for l in ca if l not in common] + [l for l in cb if l not in common]
    return sum(1 for l in path if topo.parent[l] >= 0 and topo.joint_type[l] != 0)


def case_pairs(topo, boxes, floating):
    """pairs sorted by their first box -- runs of a repeated first box -- with the world pairs of a robot box in between its robot pairs.
    Robot pairs have two moving joints between their links at least: across a single joint the overlap along the joint's axis never
    changes, across fixed joints nothing does (the reference skips those as neighbours).  A world pair needs one, or a floating base."""
    rob = [i for i, b in enumerate(boxes) if b[0] >= 0]
    wld = [i for i, b in enumerate(boxes) if b[0] < 0]
    out = []
    for i in rob:
        mine = [(i, j) for j in rob if j > i and _moving_joints(topo, boxes[i][0], boxes[j][0]) >= 2]
        wp = [(i, w) for w in wld if floating or _moving_joints(topo, boxes[i][0], -1) >= 1]
        for k in range(max(len(mine), len(wp))):  # interleaved
            out += mine[k:k + 1] + wp[k:k + 1]
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def reference_case(topo, floating, boxes, pairs, st, C, step, base_pos, mode):
    """(val, idx, bar) (C, P) the device has to meet, after the assertions on the restatement's side"""
    assert len(pairs) >= BATCH + 8
    R, c, h = br.box_world(topo, boxes, st["q"], floating, st.get("rpy"), base_pos, mode)
    want, scale = br.pair_distances(R, c, h, pairs)
    _, emu = emul_eval(topo, floating, boxes, pairs, st["q"], st.get("rpy") if floating else None, base_pos if floating else None, mode)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(emu))
    dev = float(np.abs(emu - want)[fin].max())
    bar = np.maximum(10.0 * dev, 32.0 * EPS * np.where(fin, scale, 1.0))
    assert (want[fin] > 0).mean() >= 0.1 and (want[fin] <= 0).mean() >= 0.1, ((want[fin] > 0).mean(), "overlapping / separated shares")
    val, idx = br.candidate_minimum(want, C, step)
    T = want.shape[0] // C
    w3 = np.where(np.isfinite(want), want, np.inf).reshape(C, T, -1)[:, ::step]
    b3 = bar.reshape(C, T, -1)[:, ::step]
    won = idx >= 0
    kk = np.maximum(idx, 0) // step
    cbar = np.take_along_axis(b3, kk[:, None, :], axis=1)[:, 0]
    if w3.shape[1] > 1:
        runner = np.sort(w3, axis=1)[:, 1]
        assert np.all((runner - val)[won] > 100.0 * cbar[won]), "a runner-up lies within 100 bars of the minimum: change the seed"
    return val, idx, cbar, dev


def run_case(eng, topo, floating, boxes, pairs, st, C, step, base_pos, mode, device, why, ref=None):
    """``ref``: what ``reference_case`` returned for the same arguments, when the caller has it"""
    val, idx, bar, dev = ref if ref is not None else reference_case(topo, floating, boxes, pairs, st, C, step, base_pos, mode)
    eng.set_boxes(boxes, pairs, center_in_link_axes=mode)
    s2 = {k: st[k] for k in ("q", "rpy") if k in st}
    if device:
        import torch

        got = eng.candidate_box_distances(_dev(s2), C, step, base_pos=None if base_pos is None else torch.from_numpy(base_pos).cuda())
        assert hasattr(got["dist"], "cpu")
    else:
        got = eng.candidate_box_distances(s2, C, step, base_pos=base_pos)
    got = _host(got)
    assert got["dist"].shape == val.shape and got["idx"].dtype == np.int64
    won = idx >= 0
    err = np.abs(got["dist"] - val)
    print(f"box case {why}: max |device - restatement| = {err[won].max():.3e} = {(err / bar)[won].max():.3f} bars "
          f"(emulation - restatement {dev:.3e}; smallest bar {bar[won].min():.3e})")
    assert np.array_equal(got["idx"], idx), why
    assert np.all(got["dist"][~won] == 1e10)
    assert np.all(err[won] <= bar[won]), why
    return got


def three_links_case(rng, placement, C, T, mode=True):
    from flobaroid_amd.collision import world_boxes_from_urdf

    topo = load_topo("threeLinks")
    boxes = synthetic_boxes(topo, rng, per_link=5)
    st = random_states(topo, C * T, rng, False, use_limits=True)
    _, cen, _ = br.box_world(topo, boxes, st["q"], center_in_link_axes=mode)
    floor = world_boxes_from_urdf(os.path.join(GOLDEN, "urdf", "world_kuka.urdf"), placement)["ground_link"]
    # the floor's centre lifted to the median height of the boxes on the moving links, and tilted: about half of the poses dip into it, and the second link,
    # which turns about the vertical, does not keep its depth
    lift = np.array([0.0, 0.0, float(np.median(cen[:, 5:, 2])) - floor.center[2]])
    cx, sx, cy, sy = np.cos(0.3), np.sin(0.3), np.cos(0.2), np.sin(0.2)
    tilt = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    boxes.append((-1, floor.half, floor.center + lift, tilt @ floor.rot))
    return topo, boxes, st


def left_arm_case(rng, placement, C, T):
    from flobaroid_amd.collision import world_boxes_from_urdf

    topo = load_topo("walkman_left_arm")
    boxes = synthetic_boxes(topo, rng, pad=(0.08, 0.2))  # (fat boxes: an arm's links seldom touch otherwise)
    st = random_states(topo, C * T, rng, True, use_limits=True)
    st["rpy"] = rng.uniform(-0.6, 0.6, (C * T, 3))
    wb = world_boxes_from_urdf(os.path.join(GOLDEN, "urdf", "world_walkman_suspended.urdf"), placement)
    # the arm hangs where the crane's arm and tip are: the base wanders about the tip's centre
    bp = wb["crane_tip"].center + rng.standard_normal((C * T, 3)) * 0.15
    boxes += [(-1, b.half, b.center, b.rot) for b in wb.values()]
    return topo, boxes, st, bp


@pytest.mark.parametrize("placement,mode", [("geometric", True), ("reference", False)])
def test_three_links_on_the_floor(placement, mode):
    rng = np.random.default_rng(7)
    C = 3
    for T, step in ((130, 1), (65, 3)):  # three tiles per candidate, the last with 2 live lanes; one partial tile
        topo, boxes, st = three_links_case(rng, placement, C, T, mode)
        pairs = case_pairs(topo, boxes, False)
        eng = _engine(topo, False)
        ref = reference_case(topo, False, boxes, pairs, st, C, step, None, mode)
        a = run_case(eng, topo, False, boxes, pairs, st, C, step, None, mode, False, f"threeLinks {placement} T{T} step{step} host", ref)
        b = run_case(eng, topo, False, boxes, pairs, st, C, step, None, mode, True, f"threeLinks {placement} T{T} step{step} device", ref)
        assert a["dist"].tobytes() == b["dist"].tobytes() and np.array_equal(a["idx"], b["idx"])


@pytest.mark.parametrize("placement,mode", [("geometric", False), ("reference", True)])
def test_left_arm_floating_under_the_crane(placement, mode):
    rng = np.random.default_rng(8)
    C = 3
    for T, step in ((130, 1), (65, 3)):
        topo, boxes, st, bp = left_arm_case(rng, placement, C, T)
        pairs = case_pairs(topo, boxes, True)
        eng = _engine(topo, True)
        ref = reference_case(topo, True, boxes, pairs, st, C, step, bp, mode)
        a = run_case(eng, topo, True, boxes, pairs, st, C, step, bp, mode, False, f"left arm {placement} T{T} step{step} host", ref)
        b = run_case(eng, topo, True, boxes, pairs, st, C, step, bp, mode, True, f"left arm {placement} T{T} step{step} device", ref)
        assert a["dist"].tobytes() == b["dist"].tobytes() and np.array_equal(a["idx"], b["idx"])


def random_tree_case(seed, C, T):
    rng = np.random.default_rng(seed)
    topo = random_topology(rng, int(rng.integers(6, 12)), p_fixed=0.25, branchiness=0.5, p_prismatic=0.3)
    boxes = synthetic_boxes(topo, rng, per_link=1, pad=(0.2, 0.6))
    fl = bool(seed % 2)
    st = random_states(topo, C * T, rng, fl)
    bp = rng.standard_normal((C * T, 3)) * 0.2 if fl else None
    _, p = br.link_poses(topo, st["q"], fl, st.get("rpy"), bp)
    boxes += world_boxes_near(rng, np.concatenate([x for x in p]), 4, half=(0.3, 0.8))
    return topo, fl, boxes, st, bp


@pytest.mark.parametrize("seed", [3, 4])
def test_random_trees_with_fixed_and_prismatic_joints(seed):
    C, T = 3, 130
    topo, fl, boxes, st, bp = random_tree_case(seed, C, T)
    pairs = case_pairs(topo, boxes, fl)
    eng = _engine(topo, fl)
    ref = reference_case(topo, fl, boxes, pairs, st, C, 1, bp, bool(seed % 2))
    a = run_case(eng, topo, fl, boxes, pairs, st, C, 1, bp, bool(seed % 2), True, f"random tree {seed}", ref)
    # several launches of one block each: a candidate's blocks are folded across launches, the same bits
    eng2 = _engine(topo, fl, options={"chunk_samples": 64})
    b = run_case(eng2, topo, fl, boxes, pairs, st, C, 1, bp, bool(seed % 2), True, f"random tree {seed}, one block a launch", ref)
    assert a["dist"].tobytes() == b["dist"].tobytes() and np.array_equal(a["idx"], b["idx"])


def test_nan_rows_same_bits_and_a_candidate_alone():
    rng = np.random.default_rng(7)
    C, T = 3, 130
    topo, boxes, st = three_links_case(rng, "geometric", C, T)
    pairs = case_pairs(topo, boxes, False)
    eng = _engine(topo, False)
    got = run_case(eng, topo, False, boxes, pairs, st, C, 1, None, True, True, "before the NaN rows")
    # the same bits on a second run, and with each candidate alone in its batch
    again = _host(eng.candidate_box_distances(_dev({"q": st["q"]}), C, 1))
    assert again["dist"].tobytes() == got["dist"].tobytes() and again["idx"].tobytes() == got["idx"].tobytes()
    for c in range(C):
        one = _host(eng.candidate_box_distances(_dev({"q": st["q"][c * T:(c + 1) * T]}), 1, 1))
        assert one["dist"].tobytes() == got["dist"][c:c + 1].tobytes() and one["idx"].tobytes() == got["idx"][c:c + 1].tobytes()
    # a NaN row of q never wins: knock out the winning sample of one pair per candidate, another sample has to win
    q = st["q"].copy()
    for c in range(C):
        q[c * T + got["idx"][c, 0]] = np.nan
    g2 = run_case(eng, topo, False, boxes, pairs, {"q": q}, C, 1, None, True, True, "NaN rows")
    assert np.all(g2["idx"][:, 0] != got["idx"][:, 0]) and np.all(g2["dist"][:, 0] > got["dist"][:, 0])
    # a candidate of NaNs returns 1e10 / -1, its neighbours what they returned before
    q = st["q"].copy()
    q[T:2 * T] = np.nan
    g3 = _host(eng.candidate_box_distances({"q": q}, C, 1))
    assert np.all(g3["dist"][1] == 1e10) and np.all(g3["idx"][1] == -1)
    assert g3["dist"][[0, 2]].tobytes() == got["dist"][[0, 2]].tobytes() and np.array_equal(g3["idx"][[0, 2]], got["idx"][[0, 2]])


def test_invalid_arguments_are_refused_and_the_sets_do_not_touch_each_other():
    import capsule_restatement as cr
    from flobaroid_amd._lib import FbrError

    rng = np.random.default_rng(7)
    C, T = 3, 65
    topo, boxes, st = three_links_case(rng, "geometric", C, T)
    pairs = case_pairs(topo, boxes, False)
    eng = _engine(topo, False)
    with pytest.raises(FbrError, match="code -1"):  # no box set
        eng.candidate_box_distances(st, C, 3)
    caps = cr.synthetic_capsules(topo)
    cpairs = np.array([(i, j) for i in range(len(caps)) for j in range(i + 1, len(caps))], dtype=np.int32)
    eng.set_capsules(caps, cpairs)
    want_c = _host(eng.candidate_capsule_distances({"q": st["q"]}, C, 3))
    want_b = run_case(eng, topo, False, boxes, pairs, st, C, 3, None, True, False, "set in place")
    w = len(boxes) - 1  # the floor
    rob = boxes[0]
    bad = [([(99, rob[1], rob[2], None)], np.zeros((0, 2))), ([(-2, rob[1], rob[2], np.eye(3))], np.zeros((0, 2))),  # link out of range
           (boxes, [[0, len(boxes)]]), (boxes, [[1, 1]]),                                                            # pair index, a box with itself
           (boxes + [boxes[w]], [[w, w + 1]]),                                                                       # two world boxes
           ([(0, np.array([0.1, 0.0, 0.1]), rob[2], None)] + boxes[1:], pairs),                                      # a zero half extent
           ([(0, np.array([0.1, -0.1, 0.1]), rob[2], None)] + boxes[1:], pairs),
           ([(0, np.array([0.1, np.inf, 0.1]), rob[2], None)] + boxes[1:], pairs),
           ([(0, np.array([0.1, np.nan, 0.1]), rob[2], None)] + boxes[1:], pairs),
           ([(0, rob[1], np.array([0.0, np.nan, 0.0]), None)] + boxes[1:], pairs),                                   # a non-finite centre
           ([rob] * 4097, pairs)]                                                                                    # more than FBR_MAX_BOXES
    for b, p in bad:
        with pytest.raises(FbrError, match="code -1"):
            eng.set_boxes(b, p)
    with pytest.raises(ValueError):  # a world box without its rotation (the binding; the library refuses rot = NULL the same way)
        eng.set_boxes(boxes[:w] + [(-1, boxes[w][1], boxes[w][2], None)], pairs)
    assert eng.num_box_pairs == len(pairs)  # (the set in place before a refused call stays: used again below)
    for Cx, step, S in ((0, 3, 60), (2, 0, 60), (7, 3, 60)):  # ncand < 1, step < 1, not a multiple
        with pytest.raises(FbrError, match="code -1"):
            eng.candidate_box_distances({"q": st["q"][:S]}, Cx, step)
    again = _host(eng.candidate_box_distances({"q": st["q"]}, C, 3))
    assert again["dist"].tobytes() == want_b["dist"].tobytes() and again["idx"].tobytes() == want_b["idx"].tobytes()
    # the capsule set is untouched by all of this, and replacing or clearing it leaves the boxes alone
    got_c = _host(eng.candidate_capsule_distances({"q": st["q"]}, C, 3))
    assert got_c["dist"].tobytes() == want_c["dist"].tobytes() and got_c["idx"].tobytes() == want_c["idx"].tobytes()
    eng.set_capsules([], [])
    again = _host(eng.candidate_box_distances({"q": st["q"]}, C, 3))
    assert again["dist"].tobytes() == want_b["dist"].tobytes()
    eng.set_capsules(caps, cpairs)
    eng.set_boxes(boxes, np.zeros((0, 2)))
    with pytest.raises(FbrError, match="code -1"):  # npairs = 0
        eng.candidate_box_distances(st, C, 3)
    eng.set_boxes([], [])
    with pytest.raises(FbrError, match="code -1"):  # cleared
        eng.candidate_box_distances(st, C, 3)
    got_c = _host(eng.candidate_capsule_distances({"q": st["q"]}, C, 3))
    assert got_c["dist"].tobytes() == want_c["dist"].tobytes()
    assert np.isfinite(eng.inverse_dynamics(st, topo.x_std())).all()
