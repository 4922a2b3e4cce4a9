#!/usr/bin/env python3
"""fbr_mesh_distance_gradients on the two configurations of tools/mesh_probe.py, 64 candidates x 2000 samples resident on the device:
WALK-MAN (floating base) with fullMeshLinks ['TorsoProtections'] -- every pair of the reference's list, those of the cage's 72 triangles
served as meshes -- and the left arm alone in collisionMode "full" (its nine links as meshes of 56 to 100 triangles).  ONE gradient call at
epsilon = 1e-7 over the evaluation points of candidate_collision_constraints(hulls=True) on the set with its meshes (collisionCheckStep 3,
transitions on); beside it the distance call that found the points and the hull gradient call on the same set without meshes, at the
evaluation points of the hull distances.  Per call: the device time of all its kernels (the library's profile slot "kin"), of stage B by
itself (slot "reduce"; the rest is the plain pairs' kernel, stage A and stage C together) and the host time of the blocking call; medians of
7 alternating repetitions.  The stencil points (stage B's items are points x tiles of 64 candidates) are counted by the rule of
tests/box_gradient_restatement.path_dofs.  There is no earlier implementation: the times are recorded.
python tools/mesh_grad_probe.py [--out profiles/mesh_grad_probe.json] [--only walkman_cage|left_arm_full]"""
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
from flobaroid_amd.collision import collision_set, hull_from_box, hulls_from_urdf, meshes_from_urdf, world_boxes_from_urdf  # noqa: E402
from flobaroid_amd.topology import Topology  # noqa: E402
from box_gradient_restatement import path_dofs  # noqa: E402
from box_probe import every_link_boxes  # noqa: E402
from capsule_probe import measure  # noqa: E402


def probe(eng, topo, cs, st, C, config, eps, reps):
    dev = st["q"].device
    hp, meshes = cs["hull_pairs"], cs["meshes"]
    names = list(topo.link_names)
    link = [-1 if h.link_name is None else names.index(h.link_name) for h in cs["hulls"]]
    mp = np.array([int(a) in meshes or int(b) in meshes for a, b in hp])
    S = np.array([1 + 2 * int(path_dofs(topo, link[a], link[b], False).sum()) for a, b in hp[mp]])
    points = {}
    for key, kw in (("mesh", {"meshes": meshes}), ("convex", {})):
        eng.set_hulls(cs["hulls"], hp, **kw)
        cons = exc.candidate_collision_constraints(eng, st, C, config, hulls=True)
        points[key] = ([torch.from_numpy(np.ascontiguousarray(cons[k])).to(dev) for k in ("eval_sample", "eval_scale", "eval_pose")], cons)
    ev, cons = points["mesh"]
    hv, _ = points["convex"]
    fm = lambda: eng.mesh_distance_gradients(st, C, ev[0], scale=ev[1], pose_sample=ev[2], epsilon=eps)  # noqa: E731
    fd = lambda: eng.candidate_hull_distances(st, C, 3)  # noqa: E731
    fh = lambda: eng.hull_distance_gradients(st, C, hv[0], scale=hv[1], pose_sample=hv[2], epsilon=eps)  # noqa: E731
    rm, rd, rh = [], [], []
    got = None
    for rep in range(reps + 1):  # (the first round warms up)
        eng.set_hulls(cs["hulls"], hp, meshes=meshes)
        got = fm()
        m, d = measure(eng, fm, ("kin", "reduce")), measure(eng, fd, ("kin", "reduce"))
        eng.set_hulls(cs["hulls"], hp)
        fh()
        h = measure(eng, fh, ("kin",))
        if rep:
            rm.append(m), rd.append(d), rh.append(h)
    med = lambda r, i: float(np.median([x[0][i] for x in r]))  # noqa: E731
    call = lambda r: float(np.median([x[1] for x in r]))  # noqa: E731
    live = cons["eval_sample"] >= 0
    tiles = (C + 63) // 64
    mcol = torch.from_numpy(mp).to(dev)
    return {"pairs": int(len(hp)), "pairs_with_a_mesh": int(mp.sum()), "meshes": {cs["hulls"][h].link_name: int(len(t)) for h, t in meshes.items()},
            "items": int(live.sum()), "mesh_items": int(live[:, mp].sum()), "stencil_points": int(S.sum()), "largest_stencil": int(S.max()),
            "stage_b_items": int(S.sum()) * tiles, "workspace_MB": float(S.sum() * 14 * C * 8 / 1e6),
            "nonzero_entries_of_mesh_rows": int((got["grad_q"][:, mcol] != 0).sum()),
            "share_of_mesh_items_in_contact": float((got["dist"][:, mcol][torch.from_numpy(live[:, mp]).to(dev)] == 0).double().mean()),
            "mesh_gradient": {"all_kernels_ms": med(rm, 0), "stage_b_ms": med(rm, 1), "plain_pairs_stage_a_and_stage_c_ms": med(rm, 0) - med(rm, 1),
                              "call_ms": call(rm)},
            "distance_call": {"frames_kernel_ms": med(rd, 0), "pairs_and_finish_ms": med(rd, 1), "call_ms": call(rd)},
            "hull_gradient_same_set_without_meshes": {"kernel_ms": med(rh, 0), "call_ms": call(rh)}}


def main(reps=7):
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "mesh_grad_probe.json")
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    dev = torch.device("cuda", 0)
    urdf = os.path.join(ROOT, "tests", "golden", "urdf")
    C, T, eps = 64, 2000, 1e-7
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 10}
    out = {"candidates": C, "samples": T, "step": 3, "epsilon": eps}
    if os.path.exists(out_path) and only:
        with open(out_path) as fh_:
            out.update(json.load(fh_))
    wb = world_boxes_from_urdf(os.path.join(urdf, "world_walkman_suspended.urdf"), "geometric")
    wh = {n: hull_from_box(b) for n, b in wb.items()}
    if only in (None, "walkman_cage"):
        topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_apriori.topology.json"))
        eng = Engine(topo, floating=True)
        eng.use_torch_stream()
        eng.profile_enable(True)
        boxes = every_link_boxes(topo)
        arm, _ = hulls_from_urdf(os.path.join(urdf, "walkman_left_arm.urdf"), topo.link_names)
        cage = meshes_from_urdf(os.path.join(urdf, "walkman_apriori.urdf"), ["TorsoProtections"])
        hulls = {n: arm.get(n, hull_from_box(b)) for n, b in boxes.items()}
        hulls["TorsoProtections"] = cage["TorsoProtections"].hull
        hulls = {n: hulls[n] for n in topo.link_names if n in hulls}
        cs = collision_set(topo, {}, {"collisionMode": "convex", "fullMeshLinks": ["TorsoProtections"]}, hulls=hulls, world_hulls=wh, meshes=cage)
        st_np, _ = synth_states(topo, C * T, 1, True)
        st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
        out["walkman_cage"] = probe(eng, topo, cs, st, C, config, eps, reps)
        eng.close()
    if only in (None, "left_arm_full"):
        topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_left_arm.topology.json"))
        eng = Engine(topo, floating=True)
        eng.use_torch_stream()
        eng.profile_enable(True)
        arm, _ = hulls_from_urdf(os.path.join(urdf, "walkman_left_arm.urdf"), topo.link_names)
        ms = meshes_from_urdf(os.path.join(urdf, "walkman_left_arm.urdf"), list(arm))
        cs = collision_set(topo, {}, {"collisionMode": "full"}, hulls=arm, world_hulls=wh, meshes=ms)
        st_np, _ = synth_states(topo, C * T, 1, True)
        st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
        out["left_arm_full"] = probe(eng, topo, cs, st, C, config, eps, reps)
        eng.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh_:
        json.dump(out, fh_, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
