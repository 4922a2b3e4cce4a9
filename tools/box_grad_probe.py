#!/usr/bin/env python3
"""fbr_box_distance_gradients on device-resident WALK-MAN states (floating base, 64 candidates x 2000 samples, a box on every link): one
gradient call over the evaluation points of candidate_collision_constraints (collisionCheckStep 3, transitions on) for (a) the four boxes
of the suspended world against every robot box, the 192 world pairs of capsule mode, and (b) the 991 pairs of box mode; beside each the
distance call that found the evaluation points, and the capsule gradient call on the same number of capsule pairs for scale.  Per call:
the device time of the kernel (hipEvents of the library's profile slot) and the host time of the blocking call; medians of 7 alternating
repetitions.  python tools/box_grad_probe.py [--out profiles/box_grad_probe.json]"""
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
from flobaroid_amd.collision import collision_set, world_boxes_from_urdf  # noqa: E402
from flobaroid_amd.topology import Topology  # noqa: E402
from box_probe import every_link_boxes  # noqa: E402
from capsule_probe import every_link_capsules, measure  # noqa: E402


def main(reps=7):
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "box_grad_probe.json")
    dev = torch.device("cuda", 0)
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_apriori.topology.json"))
    eng = Engine(topo, floating=True)
    eng.use_torch_stream()
    eng.profile_enable(True)
    boxes, caps = every_link_boxes(topo), every_link_capsules(topo)
    wb = world_boxes_from_urdf(os.path.join(ROOT, "tests", "golden", "urdf", "world_walkman_suspended.urdf"), "geometric")
    both = collision_set(topo, {}, {"collisionMode": "box"}, boxes=boxes, world_boxes=wb)
    world = np.array([b in wb for _, b in both["pair_names"]])
    sets = {"world_4_boxes": both["box_pairs"][world], "box_mode_robot_pairs": both["box_pairs"][~world]}
    cap_pairs = collision_set(topo, caps, {})["pairs"]
    C, T, eps = 64, 2000, 1e-7
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 10}
    st_np, _ = synth_states(topo, C * T, 1, True)
    st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
    out = {"model": "walkman_apriori", "candidates": C, "samples": T, "step": 3, "epsilon": eps, "boxes": len(both["boxes"]), "dofs": topo.num_dofs}
    for name, pairs in sets.items():
        eng.set_boxes(both["boxes"], pairs)
        eng.set_capsules(list(caps.values()), cap_pairs[: len(pairs)])
        cons = exc.candidate_collision_constraints(eng, st, C, config, boxes=True)
        ccons = exc.candidate_collision_constraints(eng, st, C, config)
        ev = [torch.from_numpy(np.ascontiguousarray(cons[k])).to(dev) for k in ("eval_sample", "eval_scale", "eval_pose")]
        cev = [torch.from_numpy(np.ascontiguousarray(ccons[k])).to(dev) for k in ("eval_sample", "eval_scale", "eval_pose")]
        fg = lambda: eng.box_distance_gradients(st, C, ev[0], scale=ev[1], pose_sample=ev[2], epsilon=eps)  # noqa: E731
        fd = lambda: eng.candidate_box_distances(st, C, 3)  # noqa: E731
        fc = lambda: eng.capsule_distance_gradients(st, C, cev[0], scale=cev[1], pose_sample=cev[2])  # noqa: E731
        got = fg()
        fd(), fc()
        rg, rd, rc = [], [], []
        for _ in range(reps):
            rg.append(measure(eng, fg, ("kin",)))
            rd.append(measure(eng, fd, ("kin", "reduce")))
            rc.append(measure(eng, fc, ("kin",)))
        med = lambda r, i: float(np.median([x[0][i] for x in r]))  # noqa: E731
        call = lambda r: float(np.median([x[1] for x in r]))  # noqa: E731
        g = got["grad_q"]
        live = cons["eval_sample"] >= 0
        entries = int((g != 0).sum())  # (stencil entries that were evaluated and are not zero: a lower bound of the evaluated ones)
        items = int(live.sum())
        out[name] = {"pairs": int(len(pairs)), "items": items, "nonzero_entries": entries,
                     "transition_items": int(((cons["idx"] < 0) & live).sum()),
                     "share_of_items_in_collision": float((cons["g"][live] < 0).mean()),
                     "grad_kernel_ms": med(rg, 0), "grad_call_ms": call(rg),
                     "us_per_item": med(rg, 0) * 1e3 / max(items, 1),
                     "distance_call": {"frames_kernel_ms": med(rd, 0), "pairs_and_finish_ms": med(rd, 1), "call_ms": call(rd)},
                     "capsule_gradients_same_count": {"pairs": int(min(len(pairs), len(cap_pairs))), "kernel_ms": med(rc, 0), "call_ms": call(rc)}}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
