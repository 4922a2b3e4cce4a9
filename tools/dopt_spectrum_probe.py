"""Cost of the step between gram_grouped and regressor_weights both ways, for C candidates x T samples with device-resident states:
  host route:   D2H of the grouped Gram, eigvalsh (terms), eigvalsh + inv (dopt_weight_matrices), H2D of Cmat;
  device route: one Engine.dopt_terms(..., weights=True) on the Gram in HBM (and, for the objective alone, without the weights).
WALK-MAN floating base and KUKA LWR4 with friction (nb = 64).  The columns are the sorted pivoted-QR columns of these trajectories' own
summed Gram: for WALK-MAN that gave nb = 200 of 480 columns in the recorded run (profiles/dopt_spectrum_probe.json), not the 213 in pivot
order of the identification problem.  Warm-up, a device synchronisation on both sides of
every timed region, medians of `reps` repetitions.  One workgroup per candidate: C of the device's compute units are busy.
python tools/dopt_spectrum_probe.py [C=64] [T=2000] [reps=20] [json_out]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scipy.linalg as sla
import torch
from flobaroid_amd import estimation as est
from flobaroid_amd import excitation as exc
from flobaroid_amd._lib import Engine
from flobaroid_amd.topology import Topology

C, T, reps = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 64), (2, 2000), (3, 20)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cus = torch.cuda.get_device_properties(0).multi_processor_count


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


out = {"C": C, "T": T, "reps": reps, "compute_units": cus}
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
    r = {"nb": nb, "Pa": int(G.shape[1]), "gram_MB": Gh.nbytes / 1e6, "cmat_MB": C * nb * nb * 8 / 1e6}
    r["gram_grouped_ms"] = med(lambda: eng.gram_grouped(st, C, out=G))
    r["host_d2h_ms"] = med(lambda: G.cpu().numpy())
    r["host_terms_eigvalsh_ms"] = med(lambda: est.d_optimality_batch_terms(Gh, ic, 1e-4))
    Cm = exc.dopt_weight_matrices(Gh, ic, 1e-4, 0.5)[0]
    r["host_weights_eigvalsh_inv_ms"] = med(lambda: exc.dopt_weight_matrices(Gh, ic, 1e-4, 0.5))
    r["host_h2d_ms"] = med(lambda: torch.from_numpy(Cm).cuda())
    r["host_route_ms"] = r["host_d2h_ms"] + r["host_terms_eigvalsh_ms"] + r["host_weights_eigvalsh_inv_ms"] + r["host_h2d_ms"]
    r["device_terms_ms"] = med(lambda: eng.dopt_terms(G, ic, 1e-4))
    r["device_terms_and_weights_ms"] = med(lambda: eng.dopt_terms(G, ic, 1e-4, scale=0.5, weights=True))
    dev = eng.dopt_terms(G, ic, 1e-4, scale=0.5, weights=True)
    nld, lm, _ = est.d_optimality_batch_terms(Gh, ic, 1e-4)
    r["max_rel_diff_neg_log_det"] = float(np.abs(dev["neg_log_det"].cpu().numpy() - nld).max() / np.abs(nld).max())
    r["max_rel_diff_cmat"] = float(np.abs(dev["Cmat"].cpu().numpy() - Cm).max() / np.abs(Cm).max())
    r["workgroups_of_compute_units"] = f"{min(C, cus)} of {cus}"
    out[name] = r
    print(name, json.dumps(r), flush=True)
    eng.close()
if len(sys.argv) > 4:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    with open(sys.argv[4], "w") as fh:
        json.dump(out, fh, indent=1)
