"""Cost of the torque rows behind the constraint and soft-cost gradients (Phase C) on the device, for WALK-MAN floating base with C x T
samples and device-resident states: fbr_torque_row_sweep (device time of its kernel, profile class id, and the blocking call) against the
route without it -- the 1 + 3 n perturbed states of every (candidate, joint) expanded in torch, fbr_inverse_dynamics_batch over them, the
joint rows gathered -- and the end-to-end time of excitation.candidate_gradients_from_coefficients.  Medians over repetitions.
python tools/constraint_gradient_probe.py [C=64] [T=2000] [reps=5]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from flobaroid_amd import excitation as exc
from flobaroid_amd._lib import Engine
from flobaroid_amd.topology import Topology

C, T, reps = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 64), (2, 2000), (3, 5)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_apriori.topology.json"))
eng = Engine(topo, floating=True)
n, rows, P = eng.n, eng.rows, eng.cols
fb, nper = rows - n, 1 + 3 * n
rng = np.random.default_rng(0)
nf = [4] * n
cands = [exc.fourier_coefficients(rng.uniform(-0.2, 0.2, (n, 4)), rng.uniform(-0.2, 0.2, (n, 4)), np.zeros(n), nf, 2 * np.pi * 0.1) for _ in range(C)]
st = exc.candidate_states(eng, cands, T, 100.0, device=True)
x_std = topo.x_std()
eps = 1e-7
sample = torch.from_numpy(rng.integers(0, T, (C, n))).cuda()


def timed(fn, cls=()):
    dev, call = [], []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        eng.profile_get()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        call.append((time.perf_counter() - t0) * 1e3)
        p = eng.profile_get()
        dev.append({k: p[k][0] for k in cls})
    return {k: float(np.median([d[k] for d in dev[1:]])) for k in cls}, float(np.median(call[1:])), out


def expanded():
    """the same numbers from fbr_inverse_dynamics_batch: every evaluation's state written out"""
    s = (torch.arange(C, device="cuda")[:, None] * T + sample).reshape(-1)
    ex = {k: v[s].repeat_interleave(nper, dim=0) for k, v in st.items()}
    item = torch.arange(C * n, device="cuda")
    for kind, key in enumerate(("q", "dq", "ddq")):
        for d in range(n):
            ex[key][item * nper + 1 + kind * n + d, d] += eps
    tau = eng.inverse_dynamics(ex, x_std)
    jn = torch.arange(n, device="cuda").repeat(C).repeat_interleave(nper)
    return tau[torch.arange(C * n * nper, device="cuda"), fb + jn].reshape(C, n, nper)


eng.profile_enable(True)
dev, call, sw = timed(lambda: eng.torque_row_sweep(st, C, sample, x_std, eps), ("id",))
print(f"{C} candidates x {T} samples, {n} joints: {C * n} rows, {C * n * nper} evaluations")
print(f"  torque_row_sweep: kernel {dev['id']:.3f} ms, call {call:.3f} ms ({C * n * nper / max(dev['id'], 1e-9) / 1e3:.2f} M evaluations/s)")
dev, call, ref = timed(expanded, ("kin", "id"))
print(f"  expanded in torch + inverse_dynamics + gather: library kernels {dev['kin'] + dev['id']:.3f} ms, whole route {call:.3f} ms, "
      f"{3 * n * nper * 8} bytes of expanded joint states per row")
print(f"  largest difference between the two: {float((sw - ref).abs().max()):.3e} (max |tau| {float(ref.abs().max()):.3e})")
eng.profile_enable(False)
names = list(topo.dof_names)
ic = np.sort(rng.choice(P, 213, replace=False))
config = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0}
_, call, _ = timed(lambda: exc.candidate_gradients_from_coefficients(eng, cands, T, 100.0, x_std, ic, topo.limits, names, config))
print(f"  candidate_gradients_from_coefficients end to end: {call:.1f} ms")
_, call, _ = timed(lambda: exc.candidate_dopt_gradient_from_coefficients(eng, cands, T, 100.0, ic))
print(f"  (of which candidate_dopt_gradient_from_coefficients alone: {call:.1f} ms)")
