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


def kuka(reps=5):
    """python tools/hull_probe.py kuka [--out profiles/hull_large_probe.json]: KUKA LWR4 (fixed base) with the hulls of its eight visual
    meshes (158 to 793 vertices, tests/golden/kuka_hulls.npz) and the floor of world_kuka.urdf, every pair of collisionMode "convex";
    64 candidates x 2409 samples at step 3 -- the recorded trajectory of the tutorial, a seeded offset and scale a candidate.  Frames,
    pairs and the whole call as above; the share of evaluations that enter the facet pass and the GJK iterations from the emulation on
    every 40th checked sample of two candidates.  Then the worst case of the kernel: two 1024-point spheres overlapping in all 64 samples
    of one block (3066^2 arc tests a sample, shared by the wave)."""
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "hull_large_probe.json")
    import hull_large_shapes as ls
    import hull_shapes as hs
    from flobaroid_amd.collision import world_hulls_from_urdf
    from test_gpu_hulls_large import emulate

    dev = torch.device("cuda", 0)
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "kuka_lwr4.topology.json"))
    eng = Engine(topo, floating=False)
    eng.use_torch_stream()
    eng.profile_enable(True)
    K = ls.kuka_hulls()
    wh = world_hulls_from_urdf(os.path.join(ROOT, "tests", "golden", "urdf", "world_kuka.urdf"), "geometric")
    hset = collision_set(topo, {}, {"collisionMode": "convex"}, hulls=K, world_hulls=wh)
    hp = hset["hull_pairs"]
    C, step = 64, 3
    base = np.load(os.path.join(ROOT, "tests", "golden", "kuka_trajectory_opt_1.npz"))["positions"]
    T = base.shape[0]
    rng = np.random.default_rng(0)
    q = np.concatenate([base * rng.uniform(0.7, 1.0) + rng.uniform(-0.2, 0.2, base.shape[1]) for _ in range(C)])
    st = {"q": torch.from_numpy(np.ascontiguousarray(q)).to(dev)}
    eng.set_hulls(hset["hulls"], hp, offset_in_link_axes=bool(hset.get("offset_in_link_axes", False)), large=True)
    f = lambda: eng.candidate_hull_distances(st, C, step)  # noqa: E731
    f()
    r = [measure(eng, f, ("kin", "reduce")) for _ in range(reps)]
    med = lambda i: float(np.median([x[0][i] for x in r]))  # noqa: E731
    ev = int(C * ((T + step - 1) // step) * len(hp))
    d = f()["dist"]
    rows = np.concatenate([c * T + np.arange(0, T, step)[::40] for c in (0, C - 1)])
    _, _, facet, iters = emulate(topo, False, hset["hulls"], hp, q[rows], bool(hset.get("offset_in_link_axes", False)))
    out = {"model": "kuka_lwr4", "candidates": C, "samples": T, "step": step, "hulls": len(hset["hulls"]), "pairs": int(len(hp)),
           "pair_names": [list(p) for p in hset["pair_names"]], "vertices": sorted(len(h.vertices) for h in hset["hulls"]), "evaluations": ev,
           "frames_kernel_ms": med(0), "pairs_and_finish_ms": med(1), "call_ms": float(np.median([x[1] for x in r])), "ns_per_evaluation": med(1) * 1e6 / ev,
           "share_of_pairs_in_collision": float((d < 0).double().mean()), "emulated_evaluations": int(iters.size),
           "share_entering_the_facet_pass": float(facet.mean()), "mean_gjk_iterations": float(iters.mean()), "most_gjk_iterations": int(iters.max())}
    # the worst case: one pair of 1024-point spheres, 64 samples, all overlapping by 1 to 9 mm
    gantry = hs.gantry()
    eng2 = Engine(gantry, floating=False)
    eng2.use_torch_stream()
    eng2.profile_enable(True)
    ball = ls.shape("sphere1024")
    eng2.set_hulls([ls.on(ball, "bed"), ls.on(ball, "carriage", np.array([-0.25, 0.0, -0.5]))], [[0, 1]], large=True)
    qw = np.stack([0.49 + np.arange(64) * 2.0 ** -13, np.arange(64) * 2.0 ** -12], axis=1)  # the carriage hull's centre at (q1, 0, q0)
    sw = {"q": torch.from_numpy(qw).to(dev)}
    fw = lambda: eng2.candidate_hull_distances(sw, 1, 1)  # noqa: E731
    dw = fw()["dist"]
    rw = [measure(eng2, fw, ("kin", "reduce")) for _ in range(3)]
    out["worst_case"] = {"hulls": "two 1024-point spheres, 3066 edges each", "samples_touching": 64, "arc_tests_per_sample": 3066 * 3066,
                         "minimum": float(dw[0, 0]), "pairs_and_finish_ms": float(np.median([x[0][1] for x in rw])),
                         "call_ms": float(np.median([x[1] for x in rw]))}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh_:
        json.dump(out, fh_, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    kuka() if len(sys.argv) > 1 and sys.argv[1] == "kuka" else main()
