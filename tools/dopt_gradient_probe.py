"""Cost of the D-optimality gradient of candidate trajectories on the device, stage by stage: device time (profile classes regressor /
gram = the weight kernel, reduce = the chain; kin) and the host time of the blocking call, medians over repetitions, for WALK-MAN floating base with C x T samples and
device-resident states; for ONE candidate also the route without fbr_regressor_weights (Engine.regressor -> host GEMM -> dopt_sensitivities
with a host W).  Prints the executed fp64 MFMA rate of the weight kernel against the 78.6 TFLOP/s peak.
python tools/dopt_gradient_probe.py [C=64] [T=2000] [reps=5] [chunk_candidates=8]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from flobaroid_amd import excitation as exc
from flobaroid_amd._lib import Engine
from flobaroid_amd.topology import Topology

C, T, reps, cc = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 64), (2, 2000), (3, 5), (4, 8)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
topo = Topology.load(os.path.join(ROOT, "flobaroid_amd", "robots", "walkman_apriori.topology.json"))
eng = Engine(topo, floating=True)
n, rows, P = eng.n, eng.rows, eng.cols
rng = np.random.default_rng(0)
nf = [4] * n
cands = [exc.fourier_coefficients(rng.uniform(-0.2, 0.2, (n, 4)), rng.uniform(-0.2, 0.2, (n, 4)), np.zeros(n), nf, 2 * np.pi * 0.1) for _ in range(C)]
st = exc.candidate_states(eng, cands, T, 100.0, device=True)
nb = 213
cols = np.sort(rng.choice(P, nb, replace=False)).astype(np.int32)
Cm = torch.from_numpy(rng.standard_normal((C, nb, nb)) * 1e-3).cuda()
eps = 1e-7


def timed(fn, cls):
    dev, call = [], []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        eng.profile_get()
        t0 = time.perf_counter()
        fn()
        call.append((time.perf_counter() - t0) * 1e3)
        p = eng.profile_get()
        dev.append({k: p[k][0] for k in cls})
    return {k: float(np.median([d[k] for d in dev[1:]])) for k in cls}, float(np.median(call[1:]))


eng.profile_enable(True)
W = torch.empty((cc * T * rows, P), dtype=torch.float64, device="cuda")
sub = {k: v[: cc * T] for k, v in st.items()}
nchunks = C / cc
dev, call = timed(lambda: eng.regressor_weights(sub, cc, Cm[:cc], cols=cols, out=W), ("kin", "regressor", "gram"))
rows_total = cc * T * rows
flop_model = 2.0 * rows_total * nb * nb
ldk = 4 * (-(-nb // 4) | 1)  # the tiling rule of csrc/fbr_weights.h: the largest of 4, 2, 1 sub-tiles of 16 rows within 72 KB of LDS
mt = next((m for m in (4, 2, 1) if 16 * m * ldk * 8 <= 72 * 1024), 1)
tiles = cc * -(-T * rows // (16 * mt))
mfma = tiles * mt * -(-nb // 16) * -(-nb // 4)
print(f"chunk of {cc} candidates x {T} samples ({rows_total} rows, W {W.numel() * 8 / 2**30:.2f} GiB); x{nchunks:g} chunks for {C} candidates")
print(f"  regressor_weights: kin {dev['kin']:.2f} ms, regressor writer {dev['regressor']:.2f} ms, weight kernel {dev['gram']:.2f} ms, call {call:.2f} ms")
print(f"  weight kernel: {flop_model / dev['gram'] / 1e9:.2f} TFLOP/s algorithmic, {mfma * 2048 / dev['gram'] / 1e9:.2f} TFLOP/s executed MFMA "
      f"({100 * mfma * 2048 / dev['gram'] / 1e9 / 78.6:.1f} % of 78.6)")
dev, call = timed(lambda: eng.fd_scores(sub, W, eps), ("regressor",))
print(f"  fd_scores: device {dev['regressor']:.2f} ms, call {call:.2f} ms ({cc * T * (1 + 3 * n) / dev['regressor'] / 1e3:.1f} M evaluations/s)")
sens = torch.randn((3, C * T, n), dtype=torch.float64, device="cuda")
A = np.stack([c["a"] for c in cands]); B = np.stack([c["b"] for c in cands])
dev, call = timed(lambda: eng.fourier_gradient([c["wf"] for c in cands], A, B, sens[0], sens[1], sens[2], T, 100.0), ("reduce",))
print(f"  fourier_gradient ({C} candidates): device {dev['reduce']:.3f} ms, call {call:.3f} ms")
# the route without fbr_regressor_weights, one candidate
one = {k: v[:T] for k, v in st.items()}
Ch = Cm[0].cpu().numpy()
t0 = time.perf_counter()
Y = eng.regressor(one).cpu().numpy()
t1 = time.perf_counter()
Wh = np.zeros_like(Y)
Wh[:, cols] = Y[:, cols] @ Ch
t2 = time.perf_counter()
exc.dopt_sensitivities(eng, {k: v.cpu().numpy() for k, v in one.items()}, Wh, eps)
t3 = time.perf_counter()
print(f"one candidate without it: regressor + D2H {1e3 * (t1 - t0):.1f} ms, host GEMM {1e3 * (t2 - t1):.1f} ms, dopt_sensitivities with host W "
      f"{1e3 * (t3 - t2):.1f} ms, total {1e3 * (t3 - t0):.1f} ms")
t0 = time.perf_counter()
Wd = eng.regressor_weights(one, 1, Cm[:1], cols=cols, out=W[: T * rows])
sc = eng.fd_scores(one, Wd, eps)
torch.cuda.synchronize()
print(f"one candidate with it: {1e3 * (time.perf_counter() - t0):.1f} ms")
