#!/usr/bin/env python3
"""fbr_hull_distance_gradients on device-resident WALK-MAN states (floating base, 64 candidates x 2000 samples) and the hull sets of
tools/hull_probe.py (a box on every link as a hull of 8 vertices, the nine links of the left arm with the hulls of their meshes): ONE
gradient call at epsilon = 1e-7 over the evaluation points of candidate_collision_constraints(hulls=True) (collisionCheckStep 3,
transitions on) for (a) the four boxes of the suspended world against every robot hull, 192 pairs, and (b) the 991 non-neighbour pairs of
robot links; beside each the hull distance call that found the evaluation points, and the box gradient call on the same pairs, boxes and
states at the evaluation points of the box distances.  Per call: the device time of the kernel (hipEvents of the library's profile slot)
and the host time of the blocking call; medians of 7 alternating repetitions.  There is no earlier implementation: the times are recorded.
python tools/hull_grad_probe.py [--out profiles/hull_grad_probe.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench import synth_states  # noqa: E402
from flobaroid_amd import excitation as exc  # noqa: E402
from flobaroid_amd._lib import Engine  # noqa: E402
from flobaroid_amd.collision import collision_set, hull_from_box, hulls_from_urdf, world_boxes_from_urdf  # noqa: E402
from flobaroid_amd.topology import Topology  # noqa: E402
from box_probe import every_link_boxes  # noqa: E402
from capsule_probe import measure  # noqa: E402


def main(reps=7):
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "hull_grad_probe.json")
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
    C, T, eps = 64, 2000, 1e-7
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 10}
    st_np, _ = synth_states(topo, C * T, 1, True)
    st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
    out = {"model": "walkman_apriori", "candidates": C, "samples": T, "step": 3, "epsilon": eps, "hulls": len(hset["hulls"]), "mesh_hulls": sorted(mesh),
           "vertices": {"min": min(len(h.vertices) for h in hset["hulls"]), "max": max(len(h.vertices) for h in hset["hulls"])}, "dofs": topo.num_dofs}
    for name, sel in (("world_4_boxes", world), ("robot_pairs", ~world)):
        hp = hset["hull_pairs"][np.sort(hset["columns"][sel, 1])]  # (still sorted by the first hull)
        bp = bset["box_pairs"][bset["columns"][sel, 1]]
        eng.set_hulls(hset["hulls"], hp)
        eng.set_boxes(bset["boxes"], bp)
        cons = exc.candidate_collision_constraints(eng, st, C, config, hulls=True)
        bcons = exc.candidate_collision_constraints(eng, st, C, config, boxes=True)
        ev = [torch.from_numpy(np.ascontiguousarray(cons[k])).to(dev) for k in ("eval_sample", "eval_scale", "eval_pose")]
        bev = [torch.from_numpy(np.ascontiguousarray(bcons[k])).to(dev) for k in ("eval_sample", "eval_scale", "eval_pose")]
        fg = lambda: eng.hull_distance_gradients(st, C, ev[0], scale=ev[1], pose_sample=ev[2], epsilon=eps)  # noqa: E731
        fd = lambda: eng.candidate_hull_distances(st, C, 3)  # noqa: E731
        fb = lambda: eng.box_distance_gradients(st, C, bev[0], scale=bev[1], pose_sample=bev[2], epsilon=eps)  # noqa: E731
        got = fg()
        fd(), fb()
        rg, rd, rb = [], [], []
        for _ in range(reps):
            rg.append(measure(eng, fg, ("kin",)))
            rd.append(measure(eng, fd, ("kin", "reduce")))
            rb.append(measure(eng, fb, ("kin",)))
        med = lambda r, i: float(np.median([x[0][i] for x in r]))  # noqa: E731
        call = lambda r: float(np.median([x[1] for x in r]))  # noqa: E731
        live = cons["eval_sample"] >= 0
        items = int(live.sum())
        out[name] = {"pairs": int(len(hp)), "items": items, "nonzero_entries": int((got["grad_q"] != 0).sum()),
                     "transition_items": int(((cons["idx"] < 0) & live).sum()), "share_of_items_in_collision": float((cons["g"][live] < 0).mean()),
                     "grad_kernel_ms": med(rg, 0), "grad_call_ms": call(rg), "us_per_item": med(rg, 0) * 1e3 / max(items, 1),
                     "distance_call": {"frames_kernel_ms": med(rd, 0), "pairs_and_finish_ms": med(rd, 1), "call_ms": call(rd)},
                     "box_gradients_same_pairs": {"kernel_ms": med(rb, 0), "call_ms": call(rb)}}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
