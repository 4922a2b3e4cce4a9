#!/usr/bin/env python3
"""fbr_suspended_base_motion on device-resident WALK-MAN states, 64 candidates x 2000 samples at 100 Hz, attachment crane_ft, damping 2000
(the values simulateTrajectory passes): device time of its two kernels -- the per-sample records (profile slot "kin") and the
one-lane-per-candidate scan ("id"; the base_acc differences are in "reduce") -- and host time of the blocking call, beside
fbr_inverse_dynamics_batch on the same states for scale and the CPU restatement's time for ONE candidate (tests/suspended_restatement.py,
form (a): the loop the reference runs through iDynTree).  Medians over alternating repetitions; one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from flobaroid_amd import excitation as exc  # noqa: E402
from flobaroid_amd._lib import Engine  # noqa: E402
import _opts  # noqa: F401,E402
from flobaroid_amd.topology import Topology  # noqa: E402


def measure(eng, fn):
    eng.profile_get()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    return {k: v[0] for k, v in eng.profile_get().items() if v[1]}, host


def main(C=64, T=2000, freq=100.0, reps=7, cpu_steps=40):
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_apriori.topology.json"))
    x = topo.x_std()
    eng = Engine(topo, floating=True)
    eng.use_torch_stream()
    eng.profile_enable(True)
    rng = np.random.default_rng(0)
    n = topo.num_dofs
    cands = [exc.fourier_coefficients([rng.standard_normal(3) * 0.1 for _ in range(n)], [rng.standard_normal(3) * 0.1 for _ in range(n)],
                                      rng.uniform(-0.05, 0.05, n), [3] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    st = exc.candidate_states(eng, cands, T, freq, device=True)
    att = list(topo.link_names).index("crane_ft")
    calls = {"suspended_base_motion": lambda: eng.suspended_base_motion(st, C, x, att, 1.0 / freq, 2000.0, with_info=True),
             "suspended_records": lambda: eng.suspended_records(st, x, att),
             "inverse_dynamics": lambda: eng.inverse_dynamics(st, x)}
    for fn in calls.values():
        fn()
    res = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            res[k].append(measure(eng, fn))
    out = {"robot": "walkman_apriori", "attachment": "crane_ft", "candidates": C, "samples_per_candidate": T, "freq": freq, "reps": reps}
    for k, runs in res.items():
        classes = sorted({c for r, _ in runs for c in r})
        out[k] = {"device_ms": {c: float(np.median([r.get(c, 0.0) for r, _ in runs])) for c in classes},
                  "call_ms": float(np.median([h for _, h in runs]))}
    info = eng.suspended_base_motion(st, C, x, att, 1.0 / freq, 2000.0, with_info=True)["info"].cpu().numpy()
    out["equilibrium_iterations_max"] = int(info[:, 0].max())
    out["clamp_events"] = int(info[:, 1].sum())
    if cpu_steps:
        import suspended_restatement as sr

        host = {k: st[k][:cpu_steps].cpu().numpy() for k in ("q", "dq", "ddq")}
        t0 = time.perf_counter()
        sr.simulate_direct(topo, att, host["q"], host["dq"], host["ddq"], 1, 1.0 / freq, 2000.0)
        dt = time.perf_counter() - t0
        out["cpu_restatement_one_candidate_s"] = {"steps_timed": cpu_steps, "seconds": dt, "extrapolated_to_T_steps": dt * T / cpu_steps}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
