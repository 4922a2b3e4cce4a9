#!/usr/bin/env python3
"""fbr_candidate_hull_distances with triangle meshes attached (fbr_model_set_hull_meshes), in the configuration of tools/hull_probe.py:
device-resident WALK-MAN states (floating base, 64 candidates x 2000 samples, collisionCheckStep 3), a box on every link as a hull of 8
vertices, the nine links of the left arm and the torso's cage with the hulls of their fixture meshes, the four boxes of the suspended
world; every pair of the reference's list.  Once as collisionMode "convex" and once with fullMeshLinks ['TorsoProtections'] (the cage's
72 triangles), on the same hulls, pairs and states, alternating; and collisionMode "full" on the left arm alone (its nine links as
meshes of 56 to 100 triangles) beside convex mode there.  Per call: the device time of the frames kernel and of the pairs + finishing
kernels (hipEvents of the library's profile slots) and the host time of the blocking call; medians of 5 alternating repetitions.  The
share of triangle evaluations the culling removes and the GJK iterations come from the g++ emulation of the same text on every 40th
checked sample of two candidates.
python tools/mesh_probe.py [--out profiles/mesh_probe.json]"""
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
from flobaroid_amd.collision import collision_set, hull_from_box, hulls_from_urdf, meshes_from_urdf, world_boxes_from_urdf  # noqa: E402
from flobaroid_amd.topology import Topology  # noqa: E402
from box_probe import every_link_boxes  # noqa: E402
from capsule_probe import measure  # noqa: E402


def compare(eng, topo, floating, convex, meshed, st, st_np, C, T, step, reps):
    """the convex set and the set with meshes on the same hulls and pairs, alternating: a dict of figures"""
    from test_hulls import emul_eval
    from test_meshes import emul_pairs

    assert convex["pair_names"] == meshed["pair_names"] and np.array_equal(convex["hull_pairs"], meshed["hull_pairs"])
    hp, meshes = meshed["hull_pairs"], meshed["meshes"]
    run = lambda: eng.candidate_hull_distances(st, C, step)  # noqa: E731
    res = {"convex": [], "mesh": []}
    dist = {}
    for rep in range(reps + 1):  # (the first round warms up)
        for key, kw in (("convex", {}), ("mesh", {"meshes": meshes})):
            eng.set_hulls(meshed["hulls"], hp, **kw)
            dist[key] = run()["dist"]
            m = measure(eng, run, ("kin", "reduce"))
            if rep:
                res[key].append(m)
    med = lambda r, i: float(np.median([x[0][i] for x in r]))  # noqa: E731
    mp = np.array([int(a) in meshes or int(b) in meshes for a, b in hp])
    rows = np.concatenate([c * T + np.arange(0, T, step)[::40] for c in (0, C - 1)])
    fr, _, _ = emul_eval(topo, floating, meshed["hulls"], hp[mp], st_np["q"][rows], st_np["rpy"][rows] if floating else None, None, False)
    _, on = emul_pairs(fr, meshed["hulls"], meshes, hp[mp], True)
    _, off = emul_pairs(fr, meshed["hulls"], meshes, hp[mp], False)
    ev = int(C * ((T + step - 1) // step))
    out = {"pairs": int(len(hp)), "pairs_with_a_mesh": int(mp.sum()), "meshes": {meshed["hulls"][h].link_name: int(len(t)) for h, t in meshes.items()},
           "checked_samples": ev, "triangle_evaluations_per_sample_before_culling": float(off[0] / len(rows)),
           "share_of_triangle_evaluations_culled": float(1.0 - on[0] / max(off[0], 1)), "most_gjk_iterations": int(max(on[2], off[2])),
           "share_of_mesh_pairs_touching": float((dist["mesh"][:, torch.from_numpy(mp).to(dist["mesh"].device)] == 0).double().mean()),
           "share_of_the_same_pairs_in_collision_as_hulls": float((dist["convex"][:, torch.from_numpy(mp).to(dist["convex"].device)] < 0).double().mean())}
    for key in ("convex", "mesh"):
        out[key] = {"frames_kernel_ms": med(res[key], 0), "pairs_and_finish_ms": med(res[key], 1), "call_ms": float(np.median([x[1] for x in res[key]]))}
    out["call_ratio_mesh_over_convex"] = out["mesh"]["call_ms"] / out["convex"]["call_ms"]
    return out


def main(reps=5):
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mesh_probe.json")
    dev = torch.device("cuda", 0)
    urdf = os.path.join(ROOT, "tests", "golden", "urdf")
    C, T, step = 64, 2000, 3
    out = {"candidates": C, "samples": T, "step": step}
    # WALK-MAN: fullMeshLinks ['TorsoProtections']
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_apriori.topology.json"))
    eng = Engine(topo, floating=True)
    eng.use_torch_stream()
    eng.profile_enable(True)
    boxes = every_link_boxes(topo)
    wb = world_boxes_from_urdf(os.path.join(urdf, "world_walkman_suspended.urdf"), "geometric")
    arm, _ = hulls_from_urdf(os.path.join(urdf, "walkman_left_arm.urdf"), topo.link_names)
    cage = meshes_from_urdf(os.path.join(urdf, "walkman_apriori.urdf"), ["TorsoProtections"])
    hulls = {n: arm.get(n, hull_from_box(b)) for n, b in boxes.items()}
    hulls["TorsoProtections"] = cage["TorsoProtections"].hull
    hulls = {n: hulls[n] for n in topo.link_names if n in hulls}
    wh = {n: hull_from_box(b) for n, b in wb.items()}
    convex = collision_set(topo, {}, {"collisionMode": "convex"}, hulls=hulls, world_hulls=wh)
    meshed = collision_set(topo, {}, {"collisionMode": "convex", "fullMeshLinks": ["TorsoProtections"]}, hulls=hulls, world_hulls=wh, meshes=cage)
    st_np, _ = synth_states(topo, C * T, 1, True)
    st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
    out["walkman_cage"] = compare(eng, topo, True, convex, meshed, st, st_np, C, T, step, reps)
    eng.close()
    # the left arm alone: collisionMode "full"
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_left_arm.topology.json"))
    eng = Engine(topo, floating=True)
    eng.use_torch_stream()
    eng.profile_enable(True)
    arm, _ = hulls_from_urdf(os.path.join(urdf, "walkman_left_arm.urdf"), topo.link_names)
    ms = meshes_from_urdf(os.path.join(urdf, "walkman_left_arm.urdf"), list(arm))
    convex = collision_set(topo, {}, {"collisionMode": "convex"}, hulls=arm, world_hulls=wh)
    full = collision_set(topo, {}, {"collisionMode": "full"}, hulls=arm, world_hulls=wh, meshes=ms)
    st_np, _ = synth_states(topo, C * T, 1, True)
    st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
    out["left_arm_full"] = compare(eng, topo, True, convex, full, st, st_np, C, T, step, reps)
    eng.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh_:
        json.dump(out, fh_, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
