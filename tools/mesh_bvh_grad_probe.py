#!/usr/bin/env python3
"""fbr_large_mesh_distance_gradients (csrc/fbr_mesh_bvh_grad.h) on KUKA LWR4 in collisionMode "full", beside tools/mesh_bvh_probe.py: which 64
entries should share a wave of the tree stage -- option mesh_grad_order, 1: candidate-major, 2: slot-major.

The set, the trajectories and the shapes are those of tools/mesh_bvh_probe.py: the eight visual meshes of tests/golden/urdf/meshes/kuka (1098
to 4434 triangles on hulls of 158 to 793 vertices) and the floor of world_kuka.urdf, 29 pairs; Fourier trajectories about a bent posture, 600
samples a candidate, collisionCheckStep 3, C = 16 (the batch of profiles/mesh_bvh_probe.json) and 64 candidates.  The gradient call runs at
the winning configurations of the collision block.

* On the GPU: the call under both orders, alternating, medians of 5 repetitions with device-resident states: the device time of the whole
  call (stage A, B, C and the plain pairs) and of the tree stage alone (hipEvents of the library's profile slots) and the host time of the
  blocking call.  The two orders are compared byte for byte.  For scale, on the same hulls, pairs and states:
  fbr_large_hull_distance_gradients in collisionMode "convex" and the distance call in collisionMode "full".
* On the CPU, in the same run after the timing (the winning configurations come from the device's collision block, so the script needs the
  card; --no-emulation leaves this part out): the g++ emulation of the traversal (tests/emul/mesh_bvh_grad_emul.cpp) with
  FbrMeshBvhStats, its packets formed exactly as the two orders form waves: node pairs wanted and triangle pairs evaluated, summed over
  all items, and the number of items.

--scale-only measures the two calls "for scale" alone: it runs on a tree that does not have the gradient call yet (the parent commit's).

python tools/mesh_bvh_grad_probe.py [--out profiles/mesh_bvh_grad_probe.json] [--no-emulation] [--scale-only]"""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from flobaroid_amd import excitation as exc  # noqa: E402
from flobaroid_amd._lib import Engine  # noqa: E402
from flobaroid_amd.collision import (FBR_MAX_LARGE_HULL_VERTICES, FBR_MAX_LARGE_MESH_TRIANGLES, collision_set, hulls_from_urdf, meshes_from_urdf,  # noqa: E402
                                     world_hulls_from_urdf)
from flobaroid_amd.topology import Topology  # noqa: E402
from capsule_probe import measure  # noqa: E402

ORDERS = {"candidate_major": 1, "slot_major": 2}


def alternate(eng, variants, run, reps):
    """{key: figures} of ``variants`` {key: callable that prepares it}, alternating; also the last result of each"""
    res, last = {k: [] for k in variants}, {}
    for rep in range(reps + 1):  # (the first round warms up)
        for key, prepare in variants.items():
            prepare()
            last[key] = run[key]() if isinstance(run, dict) else run()
            m = measure(eng, run[key] if isinstance(run, dict) else run, ("kin", "reduce"))
            if rep:
                res[key].append(m)
    out = {}
    for key, r in res.items():
        out[key] = {"device_ms": float(np.median([x[0][0] for x in r])), "distance_stage_ms": float(np.median([x[0][1] for x in r])),
                    "call_ms": float(np.median([x[1] for x in r])), "call_ms_series": [float(x[1]) for x in r]}
    return out, last


def emulate(topo, full, q_win, threads=16):
    """{order: counts} of the emulation over the MESH pairs of the set at the configurations q_win (C, P, n) in the set's own pair order"""
    import test_mesh_large_gradient as tg

    C, P, n = q_win.shape
    hp = np.asarray(full["hull_pairs"]).reshape(-1, 2)
    mode = bool(full.get("offset_in_link_axes", False))
    tg.emul()  # (built once, before the threads)

    def one(job):
        k, route = job
        _, _, ns, st = tg.tree_items(topo, full["hulls"], full["meshes"], np.tile(hp[k:k + 1], (C, 1)), q_win[:, k], mode, 1e-7, route, C=C)
        return k, route, int(ns[0]), st

    jobs = [(k, r) for k in range(P) if int(hp[k, 0]) in full["meshes"] or int(hp[k, 1]) in full["meshes"] for r in (2, 3)]
    with ThreadPoolExecutor(threads) as pool:
        done = list(pool.map(one, jobs))
    out = {}
    for name, route in (("candidate_major", 2), ("slot_major", 3)):
        mine = [d for d in done if d[1] == route]
        out[name] = {"items": int(sum(d[3]["walks"] for d in mine)), "node_pairs": int(sum(d[3]["node_pairs"] for d in mine)),
                     "leaf_pairs": int(sum(d[3]["leaf_pairs"] for d in mine)), "triangle_pairs_evaluated": int(sum(d[3]["evals"] for d in mine)),
                     "stencil_entries": int(sum(d[2] for d in mine)) * C, "mesh_pairs": len(mine)}
    return out


def main(reps=5):
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mesh_bvh_grad_probe.json")
    urdf = os.path.join(ROOT, "tests", "golden", "urdf")
    T, step, freq = 600, 3, 100.0
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "kuka_lwr4.topology.json"))
    kurdf = os.path.join(urdf, "kuka_lwr4.urdf")
    hulls, box_links = hulls_from_urdf(kurdf, topo.link_names, max_vertices=FBR_MAX_LARGE_HULL_VERTICES)
    ms = meshes_from_urdf(kurdf, list(hulls), max_triangles=FBR_MAX_LARGE_MESH_TRIANGLES)
    wh = world_hulls_from_urdf(os.path.join(urdf, "world_kuka.urdf"), "geometric")
    config = {"collisionCheckStep": step, "transitionDuration": 0.0, "collisionMode": "full"}
    convex = collision_set(topo, {}, dict(config, collisionMode="convex"), hulls=hulls, world_hulls=wh)
    full = collision_set(topo, {}, config, hulls=hulls, world_hulls=wh, meshes=ms, large_meshes=True)
    assert convex["pair_names"] == full["pair_names"] and np.array_equal(convex["hull_pairs"], full["hull_pairs"]) and not box_links
    hp = full["hull_pairs"]
    P, n = len(hp), topo.num_dofs
    sel = np.argsort(np.asarray(full["columns"])[:, 1], kind="stable")  # the set's own pair order
    eng = Engine(topo, floating=False)
    eng.use_torch_stream()
    eng.profile_enable(True)
    out = {"model": "kuka_lwr4", "pairs": int(P), "samples": T, "step": step, "meshes": {full["hulls"][h].link_name: int(len(t)) for h, t in full["meshes"].items()}}
    posture = np.array([0.3, 1.9, -0.4, -1.2, 0.5, 0.9, 0.2])
    install_full = lambda: eng.set_hulls(full["hulls"], hp, large=True, meshes=full["meshes"], large_meshes=True)  # noqa: E731
    install_convex = lambda: eng.set_hulls(full["hulls"], hp, large=True)  # noqa: E731
    for C in (16, 64):
        rng = np.random.default_rng(7)
        cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.15 for _ in range(n)], [rng.standard_normal(2) * 0.15 for _ in range(n)],
                                          posture + rng.uniform(-0.1, 0.1, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
        st = exc.candidate_states(eng, cands, T, freq, device=True)
        win = {}
        for name, cs in (("full", full), ("convex", convex)):
            cons = exc._collision_block(eng, st, C, dict(config, collisionMode=name), cs)
            win[name] = tuple(torch.from_numpy(np.ascontiguousarray(np.asarray(cons[k])[:, sel])).cuda() for k in ("eval_sample", "eval_scale", "eval_pose"))
        smp, sc, pose = win["full"]
        rec = {"candidates": C}
        if "--scale-only" not in sys.argv:
            rec = orders(eng, st, C, smp, sc, pose, install_full, reps)
        # for scale: what the parent commit has on the same hulls, pairs and states
        cs_, cc, cp = win["convex"]
        scale_figs, _ = alternate(eng, {"convex_gradient": install_convex, "full_distances": install_full},
                                  {"convex_gradient": lambda: eng.large_hull_distance_gradients(st, C, cs_, scale=cc, pose_sample=cp),
                                   "full_distances": lambda: eng.candidate_hull_distances(st, C, step)}, reps)
        rec["for_scale"] = scale_figs
        if "--no-emulation" not in sys.argv and "--scale-only" not in sys.argv:
            q = st["q"].cpu().numpy().reshape(C, T, n)
            s_h, sc_h = smp.cpu().numpy(), sc.cpu().numpy()
            q_win = q[np.arange(C)[:, None], np.maximum(s_h, 0)] * sc_h[..., None]
            rec["emulation"] = emulate(topo, full, q_win)
            e = rec["emulation"]
            rec["emulation"]["node_pair_ratio_slot_major_over_candidate_major"] = e["slot_major"]["node_pairs"] / max(e["candidate_major"]["node_pairs"], 1)
            rec["emulation"]["triangle_pair_ratio_slot_major_over_candidate_major"] = (e["slot_major"]["triangle_pairs_evaluated"]
                                                                                      / max(e["candidate_major"]["triangle_pairs_evaluated"], 1))
        out[f"C{C}"] = rec
        print(f"C = {C} done", flush=True)
    eng.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh_:
        json.dump(out, fh_, indent=1)
    print(json.dumps(out, indent=1))


def orders(eng, st, C, smp, sc, pose, install_full, reps):
    """the gradient call under both orders, alternating"""
    grad = lambda: eng.large_mesh_distance_gradients(st, C, smp, scale=sc, pose_sample=pose)  # noqa: E731
    install_full()
    figs, last = alternate(eng, {k: (lambda o=o: eng.set_option("mesh_grad_order", o)) for k, o in ORDERS.items()}, grad, reps)
    eng.set_option("mesh_grad_order", 0)
    same = bool(torch.equal(last["candidate_major"]["dist"], last["slot_major"]["dist"]) and torch.equal(last["candidate_major"]["grad_q"], last["slot_major"]["grad_q"]))
    d = last["candidate_major"]["dist"]
    rec = dict(figs, candidates=C, identical_bytes=same, share_of_centre_distances_at_zero=float((d == 0).double().mean()),
               call_ratio_slot_major_over_candidate_major=figs["slot_major"]["call_ms"] / figs["candidate_major"]["call_ms"])
    return rec


if __name__ == "__main__":
    main()
