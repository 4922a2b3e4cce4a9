#!/usr/bin/env python3
"""Cost of the gradient path under the suspended base: excitation.candidate_gradients_from_coefficients on WALK-MAN hanging from crane_ft
with damping 15 (walkman_full.yaml), no collision set, at C = 1, T = 4000 (one IPOPT callback) and C = 16, T = 2000, at 100 Hz -- without
``suspended=`` (the stationary base), with it under ``suspended_base="identity"`` and under ``"held"`` -- and the split of the difference:
the suspended scan (Engine.suspended_base_motion on the same states) beside the two sweeps at the rest base and at the swung base (the
D-optimality sweep: regressor_weights + fd_scores + fourier_gradient; the torque sweep: candidate_torque_jacobians).  Host clock around calls
that end synchronised; medians of 7 alternating repetitions after one warm-up of every variant; one JSON line per configuration.
python tools/suspended_gradient_probe.py [reps=7]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flobaroid_amd import excitation as exc  # noqa: E402
from flobaroid_amd._lib import Engine  # noqa: E402
from flobaroid_amd.topology import Topology  # noqa: E402

ATT, DAMPING, FREQ, EPS = "crane_ft", 15.0, 100.0, 1e-7


def run(eng, topo, C, T, reps):
    n, P = eng.n, eng.cols
    rng = np.random.default_rng(0)
    x = topo.x_std()
    cands = [exc.fourier_coefficients([rng.standard_normal(3) * 0.1 for _ in range(n)], [rng.standard_normal(3) * 0.1 for _ in range(n)],
                                      rng.uniform(-0.05, 0.05, n), [3] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    ic = np.sort(rng.choice(P, 213, replace=False))
    names = list(topo.dof_names)
    config = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0, "analyticalGradientEpsilon": EPS}
    sus_config = dict(config, floatingBaseAttachment="suspended")
    spec = {"attachment_frame": ATT, "damping": DAMPING, "x_std": x}
    whole = lambda cfg, **kw: exc.candidate_gradients_from_coefficients(eng, cands, T, FREQ, x, ic, topo.limits, names, cfg, **kw)  # noqa: E731
    plain = exc.candidate_states(eng, cands, T, FREQ)
    swung = exc.candidate_states(eng, cands, T, FREQ, suspended=spec)
    G = exc._host(eng.gram_grouped(swung, C))
    first = whole(sus_config, suspended=spec)
    sample = first["ag_cache"]["torque_absmax_idx"]
    dopt = lambda rest: exc._dopt_gradient(eng, swung, G, cands, T, FREQ, ic, 1e-4, 1.0, None, EPS, 1, 2**31, rest_base=rest)  # noqa: E731
    torque = lambda rest: exc.candidate_torque_jacobians(eng, swung, C, sample, x, EPS, rest_base=rest)  # noqa: E731
    calls = {"whole_stationary_base": lambda: whole(config),
             "whole_suspended_identity": lambda: whole(sus_config, suspended=spec, suspended_base="identity"),
             "whole_suspended_held": lambda: whole(sus_config, suspended=spec, suspended_base="held"),
             "suspended_scan": lambda: eng.suspended_base_motion(plain, C, x, ATT, 1.0 / FREQ, DAMPING, with_info=True),
             "dopt_sweep_rest_base": lambda: dopt(True), "dopt_sweep_swung_base": lambda: dopt(False),
             "torque_sweep_rest_base": lambda: torque(True), "torque_sweep_swung_base": lambda: torque(False)}
    for fn in calls.values():
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"robot": "walkman_apriori", "attachment": ATT, "damping": DAMPING, "candidates": C, "samples_per_candidate": T, "freq": FREQ, "reps": reps,
           "median_ms": {k: float(np.median(v)) for k, v in ms.items()}, "min_ms": {k: float(np.min(v)) for k, v in ms.items()},
           "max_ms": {k: float(np.max(v)) for k, v in ms.items()}}
    m = out["median_ms"]
    out["scan_us_per_step"] = 1e3 * m["suspended_scan"] / T
    out["scan_share_of_identity_call"] = m["suspended_scan"] / m["whole_suspended_identity"]
    out["suspended_info"] = {"equilibrium_iterations_max": int(first["suspended_info"][:, 0].max()), "clamp_events": int(first["suspended_info"][:, 1].sum())}
    return out


def main(reps=7):
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_apriori.topology.json"))
    eng = Engine(topo, floating=True)
    for C, T in ((1, 4000), (16, 2000)):
        print(json.dumps(run(eng, topo, C, T, reps)), flush=True)
    eng.close()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
