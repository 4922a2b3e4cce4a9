"""Cost of the observability analysis of C candidates x T samples with device-resident states, both ways:
  host route:   D2H of the grouped Gram, numpy.linalg.eigh of every G[cols, cols], the energy sum of the unobservable vectors;
  device route: one Engine.dopt_observability on the Gram in HBM (and with the eigenvalues and vectors written out as well).
WALK-MAN floating base and KUKA LWR4 with friction.  The columns are the sorted pivoted-QR columns of these trajectories' own summed
Gram, as in tools/dopt_spectrum_probe.py.  Warm-up, a device synchronisation on both sides of every timed region, medians of `reps`
repetitions.  One workgroup per candidate: C of the device's compute units are busy.
python tools/dopt_observability_probe.py [C=64] [T=2000] [reps=20] [json_out]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scipy.linalg as sla
import torch
from flobaroid_amd import excitation as exc
from flobaroid_amd._lib import Engine
from flobaroid_amd.topology import Topology

C, T, reps = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 64), (2, 2000), (3, 20)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cus = torch.cuda.get_device_properties(0).multi_processor_count
THR = 1e-6


def med(fn):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def host_analysis(Gh, ic):
    """eigh of every candidate and the energy of the eigenvectors below the cut"""
    M = Gh[:, ic[:, None], ic[None, :]]
    ev, V = np.linalg.eigh(M)
    un = np.maximum(ev, 0.0) < THR * THR * np.maximum(ev[:, -1:], 0.0)
    return np.sum(~un, axis=1), np.einsum("cji,ci->cj", V * V, un.astype(np.float64))


out = {"C": C, "T": T, "reps": reps, "compute_units": cus, "threshold": THR}
for name, floating, friction in (("walkman_apriori", True, False), ("kuka_lwr4", False, True)):
    topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", name + ".topology.json"))
    eng = Engine(topo, floating=floating, friction=friction)
    n = eng.n
    rng = np.random.default_rng(0)
    cands = [exc.fourier_coefficients(rng.uniform(-0.2, 0.2, (n, 4)), rng.uniform(-0.2, 0.2, (n, 4)), np.zeros(n), [4] * n, 2 * np.pi * 0.1) for _ in range(C)]
    st = exc._coefficient_states(eng, cands, T, 100.0, 0.02)
    G = eng.gram_grouped(st, C)
    Gh = G.cpu().numpy()
    R, piv = sla.qr(Gh.sum(axis=0), pivoting=True, mode="r")
    d = np.abs(np.diag(R))
    ic = np.sort(piv[: int(np.sum(d > 1e-9 * d[0]))]).astype(np.int32)
    nb = len(ic)
    r = {"nb": nb, "Pa": int(G.shape[1]), "gram_MB": Gh.nbytes / 1e6}
    r["host_d2h_ms"] = med(lambda: G.cpu().numpy())
    r["host_eigh_energy_ms"] = med(lambda: host_analysis(Gh, ic))
    r["host_route_ms"] = r["host_d2h_ms"] + r["host_eigh_energy_ms"]
    r["device_ms"] = med(lambda: eng.dopt_observability(G, ic, THR))
    r["device_with_eig_vec_ms"] = med(lambda: eng.dopt_observability(G, ic, THR, eigenvalues=True, vectors=True))
    r["device_terms_only_ms"] = med(lambda: eng.dopt_terms(G, ic, 1e-4))
    r["host_over_device"] = r["host_route_ms"] / r["device_ms"]
    dev = eng.dopt_observability(G, ic, THR, device_out=False)
    nobs, energy = host_analysis(Gh, ic)
    r["n_observable_device"] = [int(dev["n_observable"].min()), int(dev["n_observable"].max())]
    r["n_observable_equal_host"] = bool(np.array_equal(dev["n_observable"], nobs))
    r["max_energy_diff"] = float(np.abs(dev["energy"] - energy).max())
    r["status_or"] = int(np.bitwise_or.reduce(dev["status"]))
    r["min_margin"] = float(dev["margin"].min())
    r["workgroups_of_compute_units"] = f"{min(C, cus)} of {cus}"
    out[name] = r
    print(name, json.dumps(r), flush=True)
    eng.close()
if len(sys.argv) > 4:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    with open(sys.argv[4], "w") as fh:
        json.dump(out, fh, indent=1)
