"""fbr_large_hull_distance_gradients / Engine.large_hull_distance_gradients and the large_hull_gradient=True path of excitation on the
device (csrc/fbr_hull_large_grad.h: recorded poses, one distance per pose with the facet pass of a touching entry shared by the wave, the
quotients).

* (g) small hulls through two routes on the same device: set_hulls + hull_distance_gradients against set_hulls(large=True) with option
  hull_large_all = 1 + large_hull_distance_gradients, np.array_equal on dist and grad_q (the sign of a zero gap may depend on the order in
  which a maximum is taken); with hull_large_all = 0 the large route sends every pair of such a set through fbr_hull_grad_kernel: bytes.
* (h) the large gantry of tests/test_gpu_hulls_large.py (17 pairs, 11 of them large) against the emulation
  (tests/emul/hull_large_grad_emul.cpp) within 32 EPS x scale in the distance and (b+ + b-) / (2 eps), b+- = 32 EPS x scale, in the rows --
  the smaller term of the project's rule, so no restatement is needed here (tests/test_hull_large_gradient.py holds the emulation against
  Qhull); the same bytes from host and device states, on a second run, with each candidate alone, with hull_grad_tile 1, 8, 64 and 0; a
  set whose live lanes all touch; the small pairs' columns of the mixed set byte-equal to set_hulls + hull_distance_gradients.
* (i) KUKA LWR4 end to end: candidate_gradients_from_coefficients(..., large_hull_gradient=True) against the restated rows chained
  through the Fourier Jacobian.  The central difference in the optimiser's variables (E2E_STEP, E2E_FD_BAR) is not run here: its
  restatement-only pre-check takes 73 restated blocks of 64 samples with hulls of up to 793 vertices, minutes of Qhull.
* (j) refusals leave the set in place.

Measured on an MI355X ("Large convex hulls", has the table): (g) equal on every case; (h) the device returns the emulation's
bits in every entry, |delta dist| / bar = |delta grad| / bar = 0.000, 220 stencil entries a call, 0.236 of them in the facet pass at the
contacts and none beside them; the full-ballot set equal at every width; (i) rows within 0.011 of the chained bars of the restated chain,
grad_q within 0.011 bars of the restatement, 72 of the 150 stencil entries (0.48) in the facet pass; device time of the call 0.879 ms, of
stage B 0.838 ms at C = 2 and 0.869 / 0.828 ms at C = 1 (medians of 7); the automatic tile width is 1 for (i) and for C = 1 (150 and 75
entries against 12 x 256 wave slots).  The central difference of (i) in the optimiser's variables: nobody has measured it."""
import numpy as np
import pytest

import hull_gradient_restatement as hg
import hull_restatement as hr
from box_gradient_restatement import path_dofs
from test_box_gradient import T, item_arrays
from test_gpu_boxes import _dev, _engine, _host
from test_hull_gradient import gantry_case, make_case
from test_hull_large_gradient import kuka_case, large_evaluate, restated_rows_large
from test_hulls import as_tuples

pytestmark = pytest.mark.gpu
EPS = hg.EPS
SMALL = 128


def _same(a, b):
    return a["dist"].tobytes() == b["dist"].tobytes() and a["grad_q"].tobytes() == b["grad_q"].tobytes()


def _states(case, device):
    import torch

    cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    st = {"q": case["q"]} if not case["floating"] else {"q": case["q"], "rpy": case["rpy"]}
    return ({k: cu(v) for k, v in st.items()}, cu(case["bp"])) if device else (st, case["bp"])


# ---- (g) two routes on the same device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [False, True], ids=["world-axes", "link-axes"])
@pytest.mark.parametrize("robot", ["kuka_lwr4", "random"])
def test_small_hulls_through_both_routes(robot, mode):
    """make_case(robot, C=65): two tiles of candidates, the second with one live lane"""
    case = make_case(robot, C=65)
    C, P = 65, len(case["pairs"])
    rng = np.random.default_rng(22)
    small, large = _engine(case["topo"], case["floating"]), _engine(case["topo"], case["floating"], options={"hull_large_all": 1})
    small.set_hulls(case["hulls"], case["pairs"], offset_in_link_axes=mode)
    large.set_hulls(case["hulls"], case["pairs"], offset_in_link_axes=mode, large=True)
    for eps, with_scale, device in ((1e-7, True, True), (1e-4, False, False)):
        sample, scale, pose = item_arrays(case, rng, C, P, with_scale)
        st, bp = _states(case, device)
        a = _host(small.hull_distance_gradients(st, C, sample, scale=scale, pose_sample=pose, base_pos=bp, epsilon=eps))
        large.set_option("hull_large_all", 1)
        b = _host(large.large_hull_distance_gradients(st, C, sample, scale=scale, pose_sample=pose, base_pos=bp, epsilon=eps))
        assert np.array_equal(a["dist"], b["dist"]) and np.array_equal(a["grad_q"], b["grad_q"]), (robot, mode, eps)
        assert (a["dist"] <= 0).any() and (a["dist"] == hg.NONE).any() and np.abs(a["grad_q"]).max() > 1e-2
        large.set_option("hull_large_all", 0)  # read by every call: all pairs are small and go through fbr_hull_grad_kernel
        assert _same(a, _host(large.large_hull_distance_gradients(st, C, sample, scale=scale, pose_sample=pose, base_pos=bp, epsilon=eps)))
    small.close()
    large.close()


def test_gantry_contacts_through_both_routes():
    """tests/test_hull_gradient.py gantry_case: parallel faces 1e-2 apart, 1e-3 deep and exactly touching, the 128-vertex pair"""
    smp = np.zeros((1, 4), dtype=np.int64)
    small = large = None
    for kind, gap in (("stack", 1e-2), ("stack", -1e-3), ("stack", 0.0), ("round", 0.0)):
        case = gantry_case(kind, gap)
        small = small or _engine(case["topo"], False)
        large = large or _engine(case["topo"], False, options={"hull_large_all": 1})
        for mode in (False, True):
            small.set_hulls(case["hulls"], case["pairs"], offset_in_link_axes=mode)
            large.set_hulls(case["hulls"], case["pairs"], offset_in_link_axes=mode, large=True)
            for eps in (1e-7, 1e-4):
                a = small.hull_distance_gradients({"q": case["q"]}, 1, smp, epsilon=eps)
                b = large.large_hull_distance_gradients({"q": case["q"]}, 1, smp, epsilon=eps)
                assert np.array_equal(a["dist"], b["dist"]) and np.array_equal(a["grad_q"], b["grad_q"]), (kind, gap, mode, eps)
                assert np.abs(a["grad_q"]).max() > 0.1
    small.close()
    large.close()


# ---- (h) large shapes against the emulation ---------------------------------------------------------------------------------------------------
def _gantry():
    from test_gpu_hulls import GAPS, TOUCH, TT
    from test_gpu_hulls_large import large_gantry_case

    topo, hl, pairs, q = large_gantry_case()[:4]
    case = {"topo": topo, "floating": False, "hulls": hl, "pairs": pairs, "q": q, "rpy": None, "bp": None}
    return case, len(GAPS), np.array(TOUCH), TT


def _bars(case, C, sample, eps, pairs=None):
    """(dist bar (C, P), row bar (C, P, 1), on_path (P, n)): 32 EPS x scale at the evaluated configuration -- the scale of a stencil point
    differs from the centre's by eps at most, far below the bar's own resolution, so twice the centre's b over 2 eps"""
    topo, hl = case["topo"], case["hulls"]
    pairs = case["pairs"] if pairs is None else pairs
    tup = as_tuples(topo, hl)
    diam = hg.diameters(tup)
    Tn = case["q"].shape[0] // C
    rows = (np.arange(C) * Tn)[:, None] + np.maximum(sample, 0)
    b = np.zeros(sample.shape)
    for c in range(C):
        _, cen = hr.hull_world(topo, tup, case["q"][rows[c]], False, None, None, True)
        k = np.arange(len(pairs))
        b[c] = 32.0 * EPS * (hr.pair_scale(cen[k, pairs[:, 0]], diam[pairs[:, 0]], cen[k, pairs[:, 1]], diam[pairs[:, 1]]) + eps)
    on = np.array([path_dofs(topo, tup[a][0], tup[b_][0], True) for a, b_ in pairs])
    return b, (2.0 * b / (2.0 * eps))[..., None], on


def test_large_shapes_on_the_gantry_against_the_emulation():
    case, C, touch, TT = _gantry()
    pairs, P = case["pairs"], len(case["pairs"])
    nv = np.array([len(h.vertices) for h in case["hulls"]])
    big = (nv[pairs] > SMALL).any(axis=1)
    assert P == 17 and big.sum() == 11
    eng = _engine(case["topo"], False)
    eng.set_hulls(case["hulls"], pairs, offset_in_link_axes=True, large=True)
    st, dst = {"q": case["q"]}, _dev({"q": case["q"]})
    for eps in (1e-7, 1e-4):
        for shift in (0, -1):  # the configuration that reaches the gap, and its neighbour
            sample = np.repeat((touch + shift)[:, None], P, axis=1).astype(np.int64)
            ed, eg, ns, facet = large_evaluate(case, C, sample, None, None, eps, True, 1)
            bd, bg, on = _bars(case, C, sample, eps)
            a = eng.large_hull_distance_gradients(st, C, sample, epsilon=eps)
            errd, errg = np.abs(a["dist"] - ed) / bd, np.abs(a["grad_q"] - eg) / bg
            print(f"large gantry eps {eps:g} shift {shift}: {int(ns.sum())} stencil entries, {facet / ns.sum():.3f} in the facet pass; max |delta dist| / bar = "
                  f"{errd.max():.3f}, max |delta grad| / bar = {errg.max():.3f}; device == emulation in {(a['grad_q'] == eg).mean():.3f} of the entries")
            assert np.all(errd <= 1.0) and np.all(errg <= 1.0)
            assert np.all(a["grad_q"][:, ~on] == 0.0) and np.abs(a["grad_q"]).max() > 0.5  # (on the gantry both joints lie on every pair's path)
            if shift == 0:
                assert (a["dist"] <= 0).any() and (a["dist"] > 0).any() and facet > 0
            b = _host(eng.large_hull_distance_gradients(dst, C, _dev({"s": sample})["s"], epsilon=eps))
            assert _same(a, b) and _same(a, eng.large_hull_distance_gradients(st, C, sample, epsilon=eps))  # host and device states, a second run
            if eps == 1e-4:
                continue
            for k in range(C):  # a candidate alone gives the bytes of its row
                one = eng.large_hull_distance_gradients({"q": case["q"][k * TT:(k + 1) * TT]}, 1, sample[k:k + 1], epsilon=eps)
                assert one["dist"].tobytes() == a["dist"][k:k + 1].tobytes() and one["grad_q"].tobytes() == a["grad_q"][k:k + 1].tobytes()
            for width in (1, 8, 64, 0):  # the value of an entry does not depend on the tile width
                eng.set_option("hull_grad_tile", width)
                assert _same(a, eng.large_hull_distance_gradients(st, C, sample, epsilon=eps)), width
            # every pair through the stages: equal values
            eng.set_option("hull_large_all", 1)
            c = eng.large_hull_distance_gradients(st, C, sample, epsilon=eps)
            eng.set_option("hull_large_all", 0)
            assert np.array_equal(c["dist"], a["dist"]) and np.array_equal(c["grad_q"], a["grad_q"])
    eng.close()


def test_a_set_whose_lanes_all_touch():
    """one candidate 1 mm deep in the four contact columns of large hulls: every stencil entry of every pair enters the facet pass, so the
    ballot of an item is full among its live lanes -- at every tile width"""
    case, C, touch, TT = _gantry()
    hl, allp = case["hulls"], case["pairs"]
    nv = np.array([len(h.vertices) for h in hl])
    counts = {(400, 257), (1024, 256), (130, 512), (216, 793)}  # (bed, carriage) of the four contact columns of large hulls
    contact = np.array([k for k, (a, b) in enumerate(allp) if (nv[a], nv[b]) in counts and hl[a].link_name == "bed" and hl[b].link_name == "carriage"])
    assert len(contact) == 4
    pairs = np.ascontiguousarray(allp[contact])
    deep = dict(case, pairs=pairs, q=case["q"][3 * TT:4 * TT])  # the candidate of the gap -1e-3
    sample = np.full((1, 4), touch[3], dtype=np.int64)
    ed, eg, ns, facet = large_evaluate(deep, 1, sample, None, None, 1e-7, True, 1)
    # (a sphere's vertex on a sphere's vertex separates along a direction slightly off the lift: 0.9925 mm there, 1 mm on the caps)
    assert facet == ns.sum() == 20 and np.all(np.abs(ed + 1e-3) < 1e-5) and (np.abs(ed + 1e-3) < 1e-12).sum() == 3
    bd, bg, on = _bars(deep, 1, sample, 1e-7)
    eng = _engine(case["topo"], False)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, large=True)
    got = None
    for width in (0, 1, 4, 8, 64):
        eng.set_option("hull_grad_tile", width)
        a = eng.large_hull_distance_gradients({"q": deep["q"]}, 1, sample, epsilon=1e-7)
        assert np.all(np.abs(a["dist"] - ed) <= bd) and np.all(np.abs(a["grad_q"] - eg) <= bg), width
        assert got is None or _same(a, got), width
        got = a
    print(f"full ballot: max |delta dist| / bar = {(np.abs(got['dist'] - ed) / bd).max():.3f}, max |delta grad| / bar = {(np.abs(got['grad_q'] - eg) / bg).max():.3f}, "
          f"rows {got['grad_q'][0].tolist()}")
    flat = np.abs(ed[0] + 1e-3) < 1e-12
    assert np.all(np.abs(got["grad_q"][0][flat] - np.array([1.0, 0.0])) <= bg[0][flat])  # lift 1, slide 0 where a vertex rests on a cap
    eng.close()


def test_small_pairs_of_a_mixed_set_return_the_bytes_of_the_hull_gradient():
    case, C, touch, TT = _gantry()
    hl, pairs = case["hulls"], case["pairs"]
    nv = np.array([len(h.vertices) for h in hl])
    small = ~(nv[pairs] > SMALL).any(axis=1)
    keep = np.nonzero(nv <= SMALL)[0]
    new_of = {int(h): i for i, h in enumerate(keep)}
    assert small.sum() == 6 and 0 < len(keep) < len(hl)
    sample = np.repeat(touch[:, None], len(pairs), axis=1).astype(np.int64)
    sample[1, 3] = -1
    eng = _engine(case["topo"], False)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, large=True)
    mixed = eng.large_hull_distance_gradients({"q": case["q"]}, C, sample, epsilon=1e-7)
    assert mixed["dist"][1, 3] == hg.NONE and not mixed["grad_q"][1, 3].any()
    eng.set_hulls([hl[h] for h in keep], np.array([[new_of[int(a)], new_of[int(b)]] for a, b in pairs[small]], dtype=np.int32), offset_in_link_axes=True)
    alone = eng.hull_distance_gradients({"q": case["q"]}, C, np.ascontiguousarray(sample[:, small]), epsilon=1e-7)
    assert np.ascontiguousarray(mixed["dist"][:, small]).tobytes() == alone["dist"].tobytes()
    assert np.ascontiguousarray(mixed["grad_q"][:, small]).tobytes() == alone["grad_q"].tobytes() and (alone["dist"] <= 0).any()
    eng.close()


# ---- (i) KUKA end to end ------------------------------------------------------------------------------------------------------------------------
def test_kuka_large_hull_gradient_end_to_end():
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from common import load_topo
    from test_gpu_box_objectives import _cols

    topo = load_topo("kuka_lwr4")
    eng = Engine(topo, floating=False)
    case = kuka_case(lambda cands, Tn, freq: _host(exc.candidate_states(eng, cands, Tn, freq))["q"])
    cs, config, cands, q, C, Tn, freq = case["cs"], case["config"], case["cands"], case["q"], case["C"], case["T"], case["freq"]
    n, P = topo.num_dofs, len(cs["pair_names"])
    assert P == 7 and len(exc._large_hulls(cs)) == 8
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    args = (eng, cands, Tn, freq, topo.x_std(), _cols(eng, topo, False), limits, topo.dof_names, config)
    eng.profile_enable(True)
    eng.profile_get()
    full = exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0, collision=cs, large_hull_gradient=True)
    eng.profile_enable(False)
    base = exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0)
    obj = exc.candidate_objectives_from_coefficients(*args, dopt_scale=1.0, collision=cs)
    n0 = full["layout"]["collision"]
    assert n0 == base["layout"]["len"] and full["g"].shape == (C, n0 + P)
    assert np.asarray(full["f"]).tobytes() == np.asarray(base["f"]).tobytes() == np.asarray(obj["f"]).tobytes()
    assert np.ascontiguousarray(full["g"][:, :n0]).tobytes() == np.asarray(base["g"]).tobytes() and np.asarray(full["g"]).tobytes() == np.asarray(obj["g"]).tobytes()
    coll = exc.candidate_collision_gradient_from_coefficients(eng, cands, Tn, freq, config, cs, large_hull_gradient=True, hull_gradient=True)
    for k in base["obj_grad"]:
        assert np.asarray(full["obj_grad"][k]).tobytes() == np.asarray(base["obj_grad"][k]).tobytes(), k
        assert np.ascontiguousarray(full["con_grad"][k][:, :n0]).tobytes() == np.asarray(base["con_grad"][k]).tobytes(), k
        assert np.array_equal(full["con_grad"][k][:, n0:], coll["grad"][k]), k
    for kw in ({"hull_gradient": True}, {}):  # without the keyword the refusal of before
        with pytest.raises(ValueError, match=r"lwr_6_link \(793 vertices\)"):
            exc.candidate_gradients_from_coefficients(*args, dopt_scale=1.0, collision=cs, **kw)
    # the call by itself, timed: stage B inside FBR_PROF_REDUCE, the whole call inside FBR_PROF_KIN
    st = exc.candidate_states(eng, cands, Tn, freq, device=True)
    cons = exc._collision_block(eng, st, C, config, cs)
    assert np.array_equal(cons["g"], coll["g"])
    order = np.argsort(np.asarray(cs["columns"])[:, 1], kind="stable")
    ev = [np.ascontiguousarray(np.asarray(cons[k])[:, order]) for k in ("eval_sample", "eval_scale", "eval_pose")]
    eng.large_hull_distance_gradients(st, C, ev[0], scale=ev[1], pose_sample=ev[2], epsilon=1e-7)  # (warm: the workspaces exist)
    eng.profile_enable(True)
    eng.profile_get()
    dg = _host(eng.large_hull_distance_gradients(st, C, ev[0], scale=ev[1], pose_sample=ev[2], epsilon=1e-7))
    prof = eng.profile_get()
    eng.profile_enable(False)
    print(f"KUKA end to end: device time of the call {prof['kin'][0] * 1e3:.1f} us, of stage B {prof['reduce'][0] * 1e3:.1f} us (C = {C}, {P} pairs)")
    assert np.array_equal(dg["grad_q"], coll["grad_q"][:, order])
    trans = (cons["idx"] < 0) & (cons["g"] < 1e10)
    # the collision rows against the restated chain, candidate by candidate
    g = coll["grad"]
    worst = 0.0
    for c in range(C):
        flat = np.concatenate([g["wf"][c][:, None], g["q_offset"][c], g["q_range"][c], g["a"][c].reshape(P, -1), g["b"][c].reshape(P, -1)], axis=1)
        ref, want, bound = restated_rows_large(case, cons, q, cands, c, 1e-7)
        err = np.abs(flat - want)
        worst = max(worst, float((np.abs(coll["grad_q"][c] - ref["grad"][c]) / ref["bar"][c]).max()))
        print(f"KUKA end to end, candidate {c}: rows against the restated chain: max |delta| / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}, max |row| = "
              f"{np.abs(want).max():.3f}; max |delta grad_q| / bar = {worst:.3f}; {int(trans[c].sum())} of {P} pairs won by a transition configuration; "
              f"{ref['facet']} stencil entries of the block in the facet pass")
        assert np.all(err <= bound) and np.all(np.abs(coll["grad_q"][c] - ref["grad"][c]) <= ref["bar"][c]) and np.abs(flat).max() > 1e-3
        assert np.all(np.abs(coll["grad_q"][c] - ref["emul_grad"][c]) <= ref["bar"][c])
    eng.close()


# ---- (j) refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_set_in_place():
    from flobaroid_amd._lib import FbrError

    case, C, touch, TT = _gantry()
    hl, pairs = case["hulls"], case["pairs"]
    P = len(pairs)
    st, smp = {"q": case["q"]}, np.repeat(touch[:, None], P, axis=1).astype(np.int64)
    eng = _engine(case["topo"], False)
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, large=True)
    dist = lambda: _host(eng.candidate_hull_distances(st, C, 1))  # noqa: E731
    want = dist()
    good = eng.large_hull_distance_gradients(st, C, smp)

    def refused(call, msg, why):
        with pytest.raises(FbrError, match="code -1") as e:
            call()
        assert msg in str(e.value), (why, str(e.value))

    for bad in (0.0, -1e-7, float("nan"), float("inf")):
        refused(lambda: eng.large_hull_distance_gradients(st, C, smp, epsilon=bad), "fbr_large_hull_distance_gradients: epsilon", bad)
    eng.set_option("hull_grad_tile", 3)
    refused(lambda: eng.large_hull_distance_gradients(st, C, smp), "hull_grad_tile", "tile 3")
    eng.set_option("hull_grad_tile", 128)
    refused(lambda: eng.large_hull_distance_gradients(st, C, smp), "hull_grad_tile", "tile 128")
    eng.set_option("hull_grad_tile", 0)
    got = dist()
    assert got["dist"].tobytes() == want["dist"].tobytes() and got["idx"].tobytes() == want["idx"].tobytes()
    assert _same(good, eng.large_hull_distance_gradients(st, C, smp))
    # a set of set_hulls that is not large; a set with no pair
    small = [h for h in hl if len(h.vertices) <= SMALL and h.link_name]
    eng.set_hulls(small, [[0, 1]], offset_in_link_axes=True)
    want1 = dist()
    refused(lambda: eng.large_hull_distance_gradients(st, C, np.zeros((C, 1), dtype=np.int64)), "no hull set installed by fbr_model_set_large_hulls", "not large")
    got = dist()
    assert got["dist"].tobytes() == want1["dist"].tobytes() and got["idx"].tobytes() == want1["idx"].tobytes()
    eng.set_hulls(hl, np.zeros((0, 2)), offset_in_link_axes=True, large=True)
    refused(lambda: eng.large_hull_distance_gradients(st, C, np.zeros((C, 0), dtype=np.int64)), "the hull set has no pair", "no pair")
    eng.set_hulls(hl, pairs, offset_in_link_axes=True, large=True)
    got = dist()
    assert got["dist"].tobytes() == want["dist"].tobytes() and got["idx"].tobytes() == want["idx"].tobytes()
    assert _same(good, eng.large_hull_distance_gradients(st, C, smp))
    eng.close()
