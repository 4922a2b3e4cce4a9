#!/usr/bin/env python3
"""fbr_candidate_hull_distances with meshes behind a tree (fbr_model_set_large_hull_meshes, csrc/fbr_mesh_bvh.h), beside tools/mesh_probe.py:

* the left arm of WALK-MAN in collisionMode "full" (nine meshes of 56 to 100 triangles, the configuration of tools/mesh_probe.py: floating
  base, 64 candidates x 2000 samples, collisionCheckStep 3): the SAME set installed through fbr_model_set_hull_meshes (the brute-force
  kernel) and through fbr_model_set_large_hull_meshes (the tree kernel), alternating; the two results are compared byte for byte;
* KUKA LWR4 in collisionMode "full" (its eight visual meshes of 1098 to 4434 triangles on hulls of 158 to 793 vertices, the floor of
  world_kuka.urdf: 29 pairs) beside collisionMode "convex" on the same hulls (fbr_model_set_large_hulls), pairs and states -- Fourier
  trajectories about a bent posture, 16 candidates x 600 samples, collisionCheckStep 3 --, alternating.

Per call: the device time of the frames kernel and of the pairs + finishing kernels (hipEvents of the library's profile slots) and the host
time of the blocking call; medians of 5 alternating repetitions.  Per pair of KUKA, from the g++ emulation of the same text on every 25th
checked sample of the first candidate walked as ONE packet: node pairs and leaf pairs a packet, triangle pairs evaluated a sample, beside
the brute force's T_A x T_B.
python tools/mesh_bvh_probe.py [--out profiles/mesh_bvh_probe.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import synth_states  # noqa: E402
from flobaroid_amd import excitation as exc  # noqa: E402
from flobaroid_amd._lib import Engine  # noqa: E402
from flobaroid_amd.collision import (FBR_MAX_LARGE_HULL_VERTICES, FBR_MAX_LARGE_MESH_TRIANGLES, collision_set, hull_from_box, hulls_from_urdf,  # noqa: E402
                                     meshes_from_urdf, world_boxes_from_urdf, world_hulls_from_urdf)
from flobaroid_amd.topology import Topology  # noqa: E402
from capsule_probe import measure  # noqa: E402


def alternate(eng, installs, run, reps):
    """{key: figures} of the sets ``installs`` {key: callable that installs it}, alternating; also the last result of each"""
    res, last = {k: [] for k in installs}, {}
    for rep in range(reps + 1):  # (the first round warms up)
        for key, inst in installs.items():
            inst()
            last[key] = run()
            m = measure(eng, run, ("kin", "reduce"))
            if rep:
                res[key].append(m)
    out = {}
    for key, r in res.items():
        out[key] = {"frames_kernel_ms": float(np.median([x[0][0] for x in r])), "pairs_and_finish_ms": float(np.median([x[0][1] for x in r])),
                    "call_ms": float(np.median([x[1] for x in r])), "call_ms_series": [float(x[1]) for x in r]}
    return out, last


def main(reps=5):
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mesh_bvh_probe.json")
    dev = torch.device("cuda", 0)
    urdf = os.path.join(ROOT, "tests", "golden", "urdf")
    out = {}
    # ---- the left arm, collisionMode "full": one set, two kernels
    C, T, step = 64, 2000, 3
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_left_arm.topology.json"))
    eng = Engine(topo, floating=True)
    eng.use_torch_stream()
    eng.profile_enable(True)
    wh = {n: hull_from_box(b) for n, b in world_boxes_from_urdf(os.path.join(urdf, "world_walkman_suspended.urdf"), "geometric").items()}
    arm, _ = hulls_from_urdf(os.path.join(urdf, "walkman_left_arm.urdf"), topo.link_names)
    ms = meshes_from_urdf(os.path.join(urdf, "walkman_left_arm.urdf"), list(arm))
    full = collision_set(topo, {}, {"collisionMode": "full"}, hulls=arm, world_hulls=wh, meshes=ms)
    st_np, _ = synth_states(topo, C * T, 1, True)
    st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
    run = lambda: eng.candidate_hull_distances(st, C, step)  # noqa: E731
    figs, last = alternate(eng, {"brute_force": lambda: eng.set_hulls(full["hulls"], full["hull_pairs"], meshes=full["meshes"]),
                                 "tree": lambda: eng.set_hulls(full["hulls"], full["hull_pairs"], meshes=full["meshes"], large_meshes=True)}, run, reps)
    same = bool(torch.equal(last["brute_force"]["dist"], last["tree"]["dist"]) and torch.equal(last["brute_force"]["idx"], last["tree"]["idx"]))
    out["left_arm_full"] = dict(figs, candidates=C, samples=T, step=step, pairs=int(len(full["hull_pairs"])), identical_bytes=same,
                                meshes={full["hulls"][h].link_name: int(len(t)) for h, t in full["meshes"].items()},
                                call_ratio_tree_over_brute_force=figs["tree"]["call_ms"] / figs["brute_force"]["call_ms"])
    eng.close()
    # ---- KUKA LWR4, collisionMode "full" beside "convex"
    C, T, step, freq = 16, 600, 3, 100.0
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "kuka_lwr4.topology.json"))
    eng = Engine(topo, floating=False)
    eng.use_torch_stream()
    eng.profile_enable(True)
    kurdf = os.path.join(urdf, "kuka_lwr4.urdf")
    hulls, box_links = hulls_from_urdf(kurdf, topo.link_names, max_vertices=FBR_MAX_LARGE_HULL_VERTICES)
    ms = meshes_from_urdf(kurdf, list(hulls), max_triangles=FBR_MAX_LARGE_MESH_TRIANGLES)
    wh = world_hulls_from_urdf(os.path.join(urdf, "world_kuka.urdf"), "geometric")
    convex = collision_set(topo, {}, {"collisionMode": "convex"}, hulls=hulls, world_hulls=wh)
    full = collision_set(topo, {}, {"collisionMode": "full"}, hulls=hulls, world_hulls=wh, meshes=ms, large_meshes=True)
    assert convex["pair_names"] == full["pair_names"] and np.array_equal(convex["hull_pairs"], full["hull_pairs"]) and not box_links
    rng = np.random.default_rng(7)
    n = topo.num_dofs
    posture = np.array([0.3, 1.9, -0.4, -1.2, 0.5, 0.9, 0.2])
    cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.15 for _ in range(n)], [rng.standard_normal(2) * 0.15 for _ in range(n)],
                                      posture + rng.uniform(-0.1, 0.1, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    st = exc.candidate_states(eng, cands, T, freq)
    run = lambda: eng.candidate_hull_distances(st, C, step)  # noqa: E731
    hp = full["hull_pairs"]
    figs, last = alternate(eng, {"convex": lambda: eng.set_hulls(full["hulls"], hp, large=True),
                                 "full": lambda: eng.set_hulls(full["hulls"], hp, large=True, meshes=full["meshes"], large_meshes=True)}, run, reps)
    d = last["full"]["dist"]
    out["kuka_full"] = dict(figs, candidates=C, samples=T, step=step, pairs=int(len(hp)), call_ratio_full_over_convex=figs["full"]["call_ms"] / figs["convex"]["call_ms"],
                            meshes={full["hulls"][h].link_name: int(len(t)) for h, t in full["meshes"].items()},
                            share_of_mesh_minima_at_zero=float((d == 0).double().mean()),
                            share_of_the_same_pairs_in_collision_as_hulls=float((last["convex"]["dist"] < 0).double().mean()))
    # the emulation's counts, pair by pair
    import test_meshes_large as tl
    from test_gpu_meshes_large import frames_of

    q = st["q"]
    q = (q.cpu().numpy() if hasattr(q, "cpu") else np.asarray(q))[np.arange(0, T, step)[::25]]
    fr = frames_of(topo, full["hulls"], q, bool(full.get("offset_in_link_axes", False)))
    names = [h.link_name or h.name for h in full["hulls"]]
    per_pair = {}
    for k, (a, b) in enumerate(hp):
        _, sa = tl.pairs_emul(fr, full["hulls"], full["meshes"], hp[k:k + 1], True)
        per_pair[f"{names[a]} x {names[b]}"] = {"brute_force_triangle_pairs_a_sample": sa["all_pairs"] // len(q), "node_pairs_a_packet": sa["node_pairs"],
                                                "leaf_pairs_a_packet": sa["leaf_pairs"], "triangle_pairs_in_those_leaves": sa["tri_pairs"],
                                                "triangle_pairs_evaluated_a_sample": sa["evals"] / len(q), "highest_stack": sa["max_stack"],
                                                "most_gjk_iterations": sa["max_iter"]}
    out["kuka_full"]["emulation_packet_of_samples"] = int(len(q))
    out["kuka_full"]["emulation_per_pair"] = per_pair
    eng.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh_:
        json.dump(out, fh_, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
