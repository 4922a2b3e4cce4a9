"""The capsule, the box and the hull calls of one handle share their host driver and its workspaces (csrc/fbr_collision_api.hip: the
partials, the branch-point scratch, the staging of the states and the host results; the box and the hull call also the frames): calls of
the three families one after another on one Engine give the bytes each family gives on an Engine of its own."""
import numpy as np
import pytest

import capsule_restatement as cr
from common import load_topo, random_states
from test_boxes import synthetic_boxes, world_boxes_near

pytestmark = pytest.mark.gpu
C, T = 3, 130       # distances: step 1 cuts a candidate into tiles of 64, 64 and 2 checked samples, step 3 into one partial tile
CG, TG = 65, 6      # gradients: the same C * T rows as 65 candidates, a second tile of candidates with one live lane
OPTIONS = {"chunk_samples": 128}  # two blocks a launch: a candidate's tiles straddle launches, the finishing kernel carries its minimum over


def _case():
    from flobaroid_amd.collision import Box, hull_from_box

    rng = np.random.default_rng(47)
    topo = load_topo("kuka_lwr4")
    assert topo.num_dofs == 7
    q = random_states(topo, C * T, rng, False)["q"]
    rpy, bp = rng.uniform(-0.3, 0.3, (C * T, 3)), 0.1 * rng.standard_normal((C * T, 3))  # (a floating base: pose_sample picks these rows)
    L = topo.num_links
    caps = [cr.synthetic_capsules(topo, 0.04)[l] for l in (1, 3, 5, L - 1)]
    cpairs = np.array([(0, 2), (0, 3), (1, 3)], np.int32)
    sb = synthetic_boxes(topo, rng)
    boxes = [sb[2], sb[L - 2]] + world_boxes_near(rng, np.array([[0.4, 0.0, 0.5]]), 1)
    bpairs = np.array([(0, 1), (0, 2), (1, 2)], np.int32)
    hb = [sb[1], sb[L - 1]] + world_boxes_near(rng, np.array([[-0.3, 0.2, 0.6]]), 1)
    hulls = [hull_from_box(Box(topo.link_names[l] if l >= 0 else None, h, c, r, "block" if l < 0 else None)) for l, h, c, r in hb]
    hpairs = np.array([(0, 1), (0, 2), (1, 2)], np.int32)
    sample = rng.integers(-1, TG, (CG, 3)).astype(np.int64)
    sample[0, 0], sample[CG - 1, 2], sample[CG - 1, 0] = -1, -1, TG - 1
    pose = (np.maximum(sample, 0) + 1 + rng.integers(0, TG - 1, (CG, 3))) % TG
    pose[sample < 0] = -1
    return dict(topo=topo, q=q, rpy=rpy, bp=bp, caps=(caps, cpairs), boxes=(boxes, bpairs), hulls=(hulls, hpairs), sample=sample, pose=pose)


def _engine(case, families):
    from flobaroid_amd._lib import Engine

    eng = Engine(case["topo"], floating=True, options=OPTIONS)
    if "capsule" in families:
        eng.set_capsules(*case["caps"])
    if "box" in families:
        eng.set_boxes(*case["boxes"], center_in_link_axes=True)
    if "hull" in families:
        eng.set_hulls(*case["hulls"], offset_in_link_axes=True)
    return eng


def _calls(eng, case, families):
    """every call of ``families``, in the order of the shared run: {name: result}"""
    st, bp, out = {"q": case["q"], "rpy": case["rpy"]}, case["bp"], {}
    dist = {"capsule": eng.candidate_capsule_distances, "hull": eng.candidate_hull_distances, "box": eng.candidate_box_distances}
    for step in (1, 3):
        for i, fam in enumerate(("capsule", "hull", "box", "capsule")):
            if fam in families:
                out[f"dist {fam} step {step} call {i}"] = dist[fam](st, C, step, base_pos=bp)
    grad = {"capsule": lambda **kw: eng.capsule_distance_gradients(st, CG, case["sample"], base_pos=bp, **kw),
            "box": lambda **kw: eng.box_distance_gradients(st, CG, case["sample"], base_pos=bp, epsilon=1e-6, **kw),
            "hull": lambda **kw: eng.hull_distance_gradients(st, CG, case["sample"], base_pos=bp, epsilon=1e-6, **kw)}
    for pose in (None, case["pose"]):
        for fam in ("capsule", "box", "hull"):
            if fam in families:
                out[f"grad {fam} pose {'given' if pose is not None else 'none'}"] = grad[fam](pose_sample=pose)
    return out


def test_one_engine_gives_what_an_engine_per_family_gives():
    case = _case()
    shared = _calls(_engine(case, ("capsule", "box", "hull")), case, ("capsule", "box", "hull"))
    assert len(shared) == 14
    for fam in ("capsule", "box", "hull"):
        alone = _calls(_engine(case, (fam,)), case, (fam,))
        assert len(alone) == (6 if fam == "capsule" else 4)
        for name, ref in alone.items():
            got = shared[name]
            for key, a in ref.items():
                assert isinstance(a, np.ndarray) and np.array_equal(got[key], a), f"{name}: {key}"
    # the cases are what they claim to be: every distance finite with a winner inside the candidate, on a checked sample; items without
    # a sample keep 1e10 and a zero row, the others a distance and, somewhere, a slope
    for name, r in shared.items():
        if name.startswith("dist"):
            step = int(name.split()[3])
            assert np.all(np.isfinite(r["dist"])) and np.all(r["dist"] < 1e9) and np.all((r["idx"] >= 0) & (r["idx"] < T) & (r["idx"] % step == 0)), name
        else:
            none = case["sample"] < 0
            assert none.any() and np.all(r["dist"][none] == 1e10) and np.all(r["grad_q"][none] == 0.0), name
            assert np.all(np.abs(r["dist"][~none]) < 1e9) and np.any(r["grad_q"][~none] != 0.0), name
    for fam in ("box", "hull"):  # (their world members see the base move: the pose rows matter)
        assert not np.array_equal(shared[f"grad {fam} pose none"]["dist"], shared[f"grad {fam} pose given"]["dist"]), fam
