#!/usr/bin/env python3
"""fbr_candidate_extrema against fbr_inverse_dynamics_batch on the same device-resident WALK-MAN states (64 candidates x 2000 samples and
1 M samples), and candidate_objectives_from_coefficients end to end.  Per call: the device time of the launches (hipEvents of the library's
FBR_PROF_ID slot, fbr_profile_get) and the host time of the blocking call, medians over alternating repetitions."""
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
import _opts  # noqa: F401,E402
from flobaroid_amd.topology import Topology  # noqa: E402


def measure(eng, fn, reps):
    """(median device ms of the FBR_PROF_ID launches, median host ms of the call)."""
    dev, host = [], []
    for _ in range(reps):
        eng.profile_get()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(eng.profile_get()["id"][0])
    return float(np.median(dev)), float(np.median(host))


def main(reps=9):
    dev = torch.device("cuda", 0)
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_apriori.topology.json"))
    x = topo.x_std()
    out = {}
    eng = Engine(topo, floating=True)
    eng.use_torch_stream()
    eng.profile_enable(True)
    for C, T in ((64, 2000), (500, 2000)):
        S = C * T
        st_np, _ = synth_states(topo, S, 1, True)
        st = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st_np.items()}
        tau = torch.empty((S, eng.rows), dtype=torch.float64, device=dev)
        fid = lambda: eng.inverse_dynamics(st, x, out=tau)  # noqa: E731
        fex = lambda: eng.candidate_extrema(st, C, x)  # noqa: E731
        fid(), fex()  # warm-up (code objects, allocations)
        rid, rex = [], []
        for _ in range(reps):  # alternating
            rid.append(measure(eng, fid, 1))
            rex.append(measure(eng, fex, 1))
        id_dev, id_host = np.median([r[0] for r in rid]), np.median([r[1] for r in rid])
        ex_dev, ex_host = np.median([r[0] for r in rex]), np.median([r[1] for r in rex])
        # same numbers as NumPy on the torques that came back
        got = {k: v.cpu().numpy() for k, v in fex().items()}
        t3 = np.abs(np.nan_to_num(tau.cpu().numpy().reshape(C, T, -1)[..., 6:]))
        exact = bool(np.array_equal(got["tau_absmax"], t3.max(axis=1)) and np.array_equal(got["tau_absmax_idx"], t3.argmax(axis=1)))
        out[f"{C}x{T}"] = {"samples": S, "inverse_dynamics_device_ms": id_dev, "candidate_extrema_device_ms": ex_dev,
                           "device_ratio": ex_dev / id_dev, "inverse_dynamics_call_ms": id_host, "candidate_extrema_call_ms": ex_host,
                           "call_ratio": ex_host / id_host, "tau_extrema_equal_numpy": exact}
        del st, tau
    # end to end: coefficients -> states -> Gram + extrema -> objective (64 candidates x 2000 samples)
    rng = np.random.default_rng(5)
    n, nh, C, T = topo.num_dofs, 5, 64, 2000
    lim = [(topo.limits[j]["lower"], topo.limits[j]["upper"]) for j in topo.dof_names]
    cands = [exc.fourier_coefficients(0.1 * rng.standard_normal((n, nh)), 0.1 * rng.standard_normal((n, nh)), np.zeros(n), [nh] * n, 0.3,
                                      joint_limits=lim) for _ in range(C)]
    G = eng.gram(synth_states(topo, 4000, 2, True)[0])
    d = np.abs(np.linalg.qr(G)[1].diagonal())
    ic = np.flatnonzero(d > 1e-8 * d.max())
    config = {"minVelocityConstraint": False}
    run = lambda: exc.candidate_objectives_from_coefficients(eng, cands, T, 200.0, x, ic, topo.limits, topo.dof_names, config)  # noqa: E731
    run()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = run()
        ts.append((time.perf_counter() - t0) * 1e3)
    out["objectives_from_coefficients_64x2000"] = {"call_ms": float(np.median(ts)), "finite_f": int(np.isfinite(r["f"]).sum()), "candidates": C}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
