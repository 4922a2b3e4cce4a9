#!/usr/bin/env python3
"""fbr_candidate_box_distances on device-resident WALK-MAN states (floating base, 64 candidates x 2000 samples, collisionCheckStep 3, a box
on every link): (a) the four boxes of the suspended world against every robot box, (b) every non-neighbour link pair in box mode; beside
each, the same number of pairs through the capsule kernels for scale, and the NumPy restatement's time per evaluation.  Per call: the
device time of the frames kernel and of the pairs + finishing kernels (hipEvents of the library's profile slots) and the host time of the
blocking call; medians of 7 alternating repetitions.  python tools/box_probe.py [--out profiles/box_probe.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import synth_states  # noqa: E402
from flobaroid_amd._lib import Engine  # noqa: E402
from flobaroid_amd.collision import Box, collision_set, world_boxes_from_urdf  # noqa: E402
from flobaroid_amd.topology import Topology  # noqa: E402
from capsule_probe import every_link_capsules, measure  # noqa: E402


def every_link_boxes(topo, pad=0.04):
    """a box per link: around the segment from its origin to its first child's origin, `pad` wider on every side"""
    boxes = {}
    for l, name in enumerate(topo.link_names):
        ch = [c for c in range(topo.num_links) if topo.parent[c] == l]
        tip = np.array(topo.rest_p[ch[0]], dtype=float) if ch else np.array([0.0, 0.0, 0.05])
        boxes[name] = Box(name, 0.5 * np.abs(tip) + pad, 0.5 * tip)
    return boxes


def main(reps=7):
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "box_probe.json")
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
    C, T, step = 64, 2000, 3
    st_np, _ = synth_states(topo, C * T, 1, True)
    st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
    out = {"model": "walkman_apriori", "candidates": C, "samples": T, "step": step, "boxes": len(both["boxes"])}
    for name, pairs in sets.items():
        eng.set_boxes(both["boxes"], pairs)
        eng.set_capsules(list(caps.values()), cap_pairs[: len(pairs)])
        fb = lambda: eng.candidate_box_distances(st, C, step)  # noqa: E731
        fc = lambda: eng.candidate_capsule_distances(st, C, step)  # noqa: E731
        fb(), fc()
        rb, rc = [], []
        for _ in range(reps):
            rb.append(measure(eng, fb, ("kin", "reduce")))
            rc.append(measure(eng, fc, ("kin", "reduce")))
        med = lambda r, i: float(np.median([x[0][i] for x in r]))  # noqa: E731
        ev = int(C * ((T + step - 1) // step) * len(pairs))
        d = fb()["dist"]
        out[name] = {"pairs": int(len(pairs)), "evaluations": ev, "frames_kernel_ms": med(rb, 0), "pairs_and_finish_ms": med(rb, 1),
                     "call_ms": float(np.median([x[1] for x in rb])), "ns_per_evaluation": med(rb, 1) * 1e6 / ev,
                     "share_of_pairs_in_collision": float((d < 0).double().mean()),
                     "capsules_same_count": {"pairs": int(min(len(pairs), len(cap_pairs))), "points_kernel_ms": med(rc, 0),
                                             "pairs_and_finish_ms": med(rc, 1), "call_ms": float(np.median([x[1] for x in rc]))}}
    # the NumPy restatement on this host: per evaluation, on 40 samples of the world pairs
    import box_restatement as br
    from box_collision_restatement import index_boxes

    q, rpy = st_np["q"][:40], st_np["rpy"][:40]
    ib = index_boxes(topo, both["boxes"])
    t0 = time.perf_counter()
    R, c, h = br.box_world(topo, ib, q, True, rpy)
    br.pair_distances(R, c, h, sets["world_4_boxes"])
    out["numpy_restatement_us_per_evaluation"] = (time.perf_counter() - t0) * 1e6 / (40 * len(sets["world_4_boxes"]))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
