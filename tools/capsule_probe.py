#!/usr/bin/env python3
"""fbr_candidate_capsule_distances beside fbr_candidate_extrema on the same device-resident WALK-MAN states (floating base; 64 and 500
candidates x 2000 samples; collisionCheckStep 3 and 1; a few hundred pairs from collision_pairs with collisionMaxKinematicDistance, and all
1 081 non-neighbour pairs of a capsule on every link; one pair = the positions-only walk alone), candidate_objectives_from_coefficients
with and without the collision block, and the host loop the device call replaces (a scalar capsule distance per call x calls per batch).
Per call: the device time of the launches (hipEvents of the library's profile slots) and the host time of the blocking call, medians over
alternating repetitions."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_states  # noqa: E402
from flobaroid_amd import excitation as exc  # noqa: E402
from flobaroid_amd._lib import Engine  # noqa: E402
from flobaroid_amd.collision import Capsule, collision_set  # noqa: E402
import _opts  # noqa: F401,E402
from flobaroid_amd.topology import Topology  # noqa: E402


def every_link_capsules(topo, radius=0.03):
    """a capsule per link: from its origin to its first child's origin (a leaf: 5 cm along z)"""
    caps = {}
    for l, name in enumerate(topo.link_names):
        ch = [c for c in range(topo.num_links) if topo.parent[c] == l]
        caps[name] = Capsule(name, np.zeros(3), np.array(topo.rest_p[ch[0]], dtype=float) if ch else np.array([0.0, 0.0, 0.05]), radius)
    return caps


def scalar_capsule_distance(a0, a1, b0, b1, ra, rb):
    """one capsule distance the way a host loop evaluates it (3-vectors, one pair per call)"""
    d1, d2, r = a1 - a0, b1 - b0, a0 - b0
    a, e, f = float(d1 @ d1), float(d2 @ d2), float(d2 @ r)
    if a <= 1e-10 and e <= 1e-10:
        return float(np.sqrt(r @ r)) - ra - rb
    if a <= 1e-10:
        s, t = 0.0, min(max(f / e, 0.0), 1.0)
    else:
        c = float(d1 @ r)
        if e <= 1e-10:
            t, s = 0.0, min(max(-c / a, 0.0), 1.0)
        else:
            b = float(d1 @ d2)
            den = a * e - b * b
            s = min(max((b * f - c * e) / den, 0.0), 1.0) if den > 1e-10 else 0.0
            t = (b * s + f) / e
            if t < 0.0:
                t, s = 0.0, min(max(-c / a, 0.0), 1.0)
            elif t > 1.0:
                t, s = 1.0, min(max((b - c) / a, 0.0), 1.0)
    v = (a0 + s * d1) - (b0 + t * d2)
    return float(np.sqrt(v @ v)) - ra - rb


def measure(eng, fn, keys):
    eng.profile_get()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    p = eng.profile_get()
    return [p[k][0] for k in keys], host


def main(reps=7):
    dev = torch.device("cuda", 0)
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_apriori.topology.json"))
    x = topo.x_std()
    eng = Engine(topo, floating=True)
    eng.use_torch_stream()
    eng.profile_enable(True)
    caps = every_link_capsules(topo)
    sets = {"all_pairs": collision_set(topo, caps, {}), "kin_distance_4": collision_set(topo, caps, {"collisionMaxKinematicDistance": 4}),
            "one_pair": None}
    sets["one_pair"] = dict(sets["all_pairs"], pairs=sets["all_pairs"]["pairs"][:1])
    out = {"pairs": {k: int(len(v["pairs"])) for k, v in sets.items()}, "capsules": len(caps)}
    for C, T in ((64, 2000), (500, 2000)):
        S = C * T
        st_np, _ = synth_states(topo, S, 1, True)
        st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
        fex = lambda: eng.candidate_extrema(st, C, x)  # noqa: E731
        fex()
        row = {}
        for name, cs in sets.items():
            eng.set_capsules(cs["capsules"], cs["pairs"])
            for step in (3, 1):
                fc = lambda: eng.candidate_capsule_distances(st, C, step)  # noqa: E731
                fc()
                rc, rx = [], []
                for _ in range(reps):
                    rc.append(measure(eng, fc, ("kin", "reduce")))
                    rx.append(measure(eng, fex, ("id",)))
                walk, prs = np.median([r[0][0] for r in rc]), np.median([r[0][1] for r in rc])
                ex_dev, ex_host = np.median([r[0][0] for r in rx]), np.median([r[1] for r in rx])
                row[f"{name}_step{step}"] = {"points_kernel_ms": walk, "pairs_and_finish_ms": prs, "device_ms": walk + prs,
                                             "call_ms": float(np.median([r[1] for r in rc])), "extrema_device_ms": ex_dev, "extrema_call_ms": ex_host,
                                             "device_ratio_to_extrema": (walk + prs) / ex_dev,
                                             "evaluations": int(C * ((T + step - 1) // step) * len(cs["pairs"]))}
        out[f"{C}x{T}"] = row
        del st
    # end to end: coefficients -> states -> Gram + extrema (+ collision block) -> objective, 64 candidates x 2000 samples
    rng = np.random.default_rng(5)
    n, nh, C, T = topo.num_dofs, 5, 64, 2000
    lim = [(topo.limits[j]["lower"], topo.limits[j]["upper"]) for j in topo.dof_names]
    cands = [exc.fourier_coefficients(0.1 * rng.standard_normal((n, nh)), 0.1 * rng.standard_normal((n, nh)), np.zeros(n), [nh] * n, 0.3,
                                      joint_limits=lim) for _ in range(C)]
    G = eng.gram(synth_states(topo, 4000, 2, True)[0])
    d = np.abs(np.linalg.qr(G)[1].diagonal())
    ic = np.flatnonzero(d > 1e-8 * d.max())
    config = {"minVelocityConstraint": False}
    e2e = {}
    for name, cs in (("without", None), ("kin_distance_4", sets["kin_distance_4"]), ("all_pairs", sets["all_pairs"])):
        run = lambda: exc.candidate_objectives_from_coefficients(eng, cands, T, 200.0, x, ic, topo.limits, topo.dof_names, config, collision=cs)  # noqa: E731
        run()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = run()
            ts.append((time.perf_counter() - t0) * 1e3)
        e2e[name] = {"call_ms": float(np.median(ts)), "g_len": int(r["g"].shape[1])}
    out["objectives_from_coefficients_64x2000"] = e2e
    # the host loop this replaces: one scalar distance per (checked sample, pair)
    pts = rng.standard_normal((2000, 4, 3))
    t0 = time.perf_counter()
    for p in pts:
        scalar_capsule_distance(p[0], p[1], p[2], p[3], 0.03, 0.03)
    us = (time.perf_counter() - t0) / len(pts) * 1e6
    calls = 64 * ((2000 + 2) // 3) * out["pairs"]["all_pairs"]
    out["host_loop"] = {"us_per_scalar_distance": us, "calls_64x2000_step3_all_pairs": calls, "seconds": us * calls * 1e-6}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
