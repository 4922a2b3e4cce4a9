#!/usr/bin/env python3
"""fbr_candidate_hull_distances on device-resident WALK-MAN states (floating base, 64 candidates x 2000 samples, collisionCheckStep 3): a box
on every link as a hull of 8 vertices -- the full set of the robot's collision meshes is no fixture --, the nine links of the left arm
with the hulls of their meshes (30 to 52 vertices); (a) the four boxes of the suspended world against every robot hull, (b) every
non-neighbour pair of robot links.  Beside each, the box kernel on the same boxes, pairs and states in the same session (the yardstick).  Per call:
the device time of the frames kernel and of the pairs + finishing kernels (hipEvents of the library's profile slots) and the host time of
the blocking call; medians of 5 alternating repetitions.  The share of evaluations that enter the facet pass and the largest number of GJK
iterations come from the g++ emulation of the same text on every 40th checked sample of two candidates.
python tools/hull_probe.py [--out profiles/hull_probe.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import synth_states  # noqa: E402
from flobaroid_amd._lib import Engine  # noqa: E402
from flobaroid_amd.collision import collision_set, hull_from_box, hulls_from_urdf, world_boxes_from_urdf  # noqa: E402
from flobaroid_amd.topology import Topology  # noqa: E402
from box_probe import every_link_boxes  # noqa: E402
from capsule_probe import measure  # noqa: E402


def main(reps=5):
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "hull_probe.json")
    dev = torch.device("cuda", 0)
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_apriori.topology.json"))
    eng = Engine(topo, floating=True)
    eng.use_torch_stream()
    eng.profile_enable(True)
    urdf = os.path.join(ROOT, "tests", "golden", "urdf")
    boxes = every_link_boxes(topo)
    wb = world_boxes_from_urdf(os.path.join(urdf, "world_walkman_suspended.urdf"), "geometric")
    mesh, _ = hulls_from_urdf(os.path.join(urdf, "walkman_left_arm.urdf"), topo.link_names)
    hulls = {n: mesh.get(n, hull_from_box(b)) for n, b in boxes.items()}
    wh = {n: hull_from_box(b) for n, b in wb.items()}
    bset = collision_set(topo, {}, {"collisionMode": "box"}, boxes=boxes, world_boxes=wb)
    hset = collision_set(topo, {}, {"collisionMode": "convex"}, hulls=hulls, world_hulls=wh)
    assert bset["pair_names"] == hset["pair_names"]
    world = np.array([b in wb for _, b in hset["pair_names"]])
    C, T, step = 64, 2000, 3
    st_np, _ = synth_states(topo, C * T, 1, True)
    st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
    out = {"model": "walkman_apriori", "candidates": C, "samples": T, "step": step, "hulls": len(hset["hulls"]), "mesh_hulls": sorted(mesh),
           "vertices": {"min": min(len(h.vertices) for h in hset["hulls"]), "max": max(len(h.vertices) for h in hset["hulls"])}}
    from test_hulls import emul_eval

    rows = np.concatenate([c * T + np.arange(0, T, step)[::40] for c in (0, C - 1)])
    for name, sel in (("world_4_boxes", world), ("robot_pairs", ~world)):
        hp = hset["hull_pairs"][np.sort(hset["columns"][sel, 1])]  # (still sorted by the first hull)
        bp = bset["box_pairs"][bset["columns"][sel, 1]]
        eng.set_hulls(hset["hulls"], hp)
        eng.set_boxes(bset["boxes"], bp)
        fh = lambda: eng.candidate_hull_distances(st, C, step)  # noqa: E731
        fb = lambda: eng.candidate_box_distances(st, C, step)  # noqa: E731
        fh(), fb()
        rh, rb = [], []
        for _ in range(reps):
            rh.append(measure(eng, fh, ("kin", "reduce")))
            rb.append(measure(eng, fb, ("kin", "reduce")))
        med = lambda r, i: float(np.median([x[0][i] for x in r]))  # noqa: E731
        ev = int(C * ((T + step - 1) // step) * len(hp))
        d = fh()["dist"]
        _, _, iters = emul_eval(topo, True, hset["hulls"], hp, st_np["q"][rows], st_np["rpy"][rows], None, False)
        out[name] = {"pairs": int(len(hp)), "evaluations": ev, "frames_kernel_ms": med(rh, 0), "pairs_and_finish_ms": med(rh, 1),
                     "call_ms": float(np.median([x[1] for x in rh])), "ns_per_evaluation": med(rh, 1) * 1e6 / ev,
                     "share_of_pairs_in_collision": float((d < 0).double().mean()),
                     "emulated_evaluations": int(iters.size), "share_entering_the_facet_pass": float((iters >= 1000).mean()),
                     "most_gjk_iterations": int((iters % 1000).max()), "mean_gjk_iterations": float((iters % 1000).mean()),
                     "box_kernel_same_pairs": {"frames_kernel_ms": med(rb, 0), "pairs_and_finish_ms": med(rb, 1),
                                               "call_ms": float(np.median([x[1] for x in rb]))}}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh_:
        json.dump(out, fh_, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
