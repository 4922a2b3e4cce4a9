"""An independent NumPy restatement of the capsule distance gradient (fbr_capsule_distance_gradients) and of the chain with the position
Jacobian of the trajectory series (fbr_fourier_position_chain) -- what the tests hold the HIP-free text of csrc/fbr_capsule_grad.h and the
device against.  No code shared with the kernels: link poses and the Jacobian columns come from tests/np_dynamics.world_kinematics (the
velocity of every link for dq = e_j), closest points from tests/capsule_restatement.segment_distance, the series' Jacobian from
tests/fourier_gradient_restatement.py.

    d dist / d q_j = n . (v_A - v_B),   v_X = v_link + omega_link x (p_X - o_link)   for dq = e_j,   n = (p_A - p_B) / |p_A - p_B|

(zero where |p_A - p_B| < 1e-12): the true derivative, v + omega x r.  The reference's capsule.py _point_jacobian forms v + r x omega."""
import numpy as np

import capsule_restatement as cr
import fourier_gradient_restatement as frest
from np_dynamics import rpy_R, world_kinematics

COINCIDENT = 1e-12


def path_dofs(topo, la, lb):
    """bool (n,): the joints on the tree path between links la and lb (above exactly one of them)"""
    anc = topo.ancestors_dofs()
    on = np.zeros(topo.num_dofs, dtype=bool)
    for d in set(anc[la]) ^ set(anc[lb]):
        on[d] = True
    return on


def item_gradients(topo, capsules, item_pairs, q, floating=False, rpy=None, base_pos=None):
    """One capsule pair per configuration: item_pairs (M, 2) capsule indices, q (M, n) [, rpy, base_pos (M, 3)] -> dict of dist (M,) (minus
    the radii), grad (M, n) (exact zeros off the pair's path), s, t, branch, near, cond (capsule_restatement.parameter_condition), on_path
    (M, n) and ``scale`` = max(1, largest |world coordinate| of the end points involved)."""
    q = np.asarray(q, dtype=np.float64)
    M, n = q.shape
    item_pairs = np.asarray(item_pairs).reshape(M, 2)
    z = np.zeros((M, 3))
    if floating and rpy is not None:
        R0 = np.transpose(rpy_R(np.asarray(rpy, dtype=np.float64)), (0, 2, 1))
        pb = z if base_pos is None else np.asarray(base_pos, dtype=np.float64)
    else:
        R0, pb = np.tile(np.eye(3), (M, 1, 1)), z
    kin = world_kinematics(topo, q, 0 * q, 0 * q, R0, z, z, z, z, p_b=pb)
    link = np.array([c[0] for c in capsules])
    p0 = np.array([c[1] for c in capsules], dtype=np.float64)
    p1 = np.array([c[2] for c in capsules], dtype=np.float64)
    rad = np.array([c[3] for c in capsules], dtype=np.float64)
    rows = np.arange(M)

    def world(ci):
        l = link[ci]
        R, o = kin["R"][l, rows], kin["p"][l, rows]
        return l, o, np.einsum("mij,mj->mi", R, p0[ci]) + o, np.einsum("mij,mj->mi", R, p1[ci]) + o

    la, oa, a0, a1 = world(item_pairs[:, 0])
    lb, ob, b0, b1 = world(item_pairs[:, 1])
    sd = cr.segment_distance(a0, a1, b0, b1)
    pa = a0 + sd["s"][:, None] * (a1 - a0)
    pbp = b0 + sd["t"][:, None] * (b1 - b0)
    diff = pa - pbp
    with np.errstate(invalid="ignore", divide="ignore"):
        nv = np.where((sd["dist"] < COINCIDENT)[:, None], 0.0, diff / sd["dist"][:, None])
    grad = np.zeros((M, n))
    for j in range(n):
        e = np.zeros_like(q)
        e[:, j] = 1.0
        kj = world_kinematics(topo, q, e, 0 * q, R0, z, z, z, z, p_b=pb)
        va = kj["v"][la, rows] + np.cross(kj["w"][la, rows], pa - oa)
        vb = kj["v"][lb, rows] + np.cross(kj["w"][lb, rows], pbp - ob)
        grad[:, j] = np.einsum("mi,mi->m", nv, va - vb)
    on = np.zeros((M, n), dtype=bool)
    cache = {}
    for i in range(M):
        key = (int(la[i]), int(lb[i]))
        if key not in cache:
            cache[key] = path_dofs(topo, *key)
        on[i] = cache[key]
    grad = np.where(on, grad, 0.0)
    ep = np.concatenate([a0, a1, b0, b1], axis=1)
    return {"dist": sd["dist"] - rad[item_pairs[:, 0]] - rad[item_pairs[:, 1]], "grad": grad, "s": sd["s"], "t": sd["t"], "branch": sd["branch"],
            "near": sd["near"], "cond": cr.parameter_condition(a0, a1, b0, b1), "on_path": on, "scale": max(1.0, cr.world_scale(ep))}


def distance_gradient(topo, capsules, pairs, q, floating=False, rpy=None, base_pos=None):
    """every pair at every configuration: q (S, n) -> item_gradients' arrays reshaped to (S, P[, n])"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    S, P = q.shape[0], pairs.shape[0]
    rep = lambda a: None if a is None else np.repeat(np.asarray(a, dtype=np.float64), P, axis=0)  # noqa: E731
    out = item_gradients(topo, capsules, np.tile(pairs, (S, 1)), rep(q), floating, rep(rpy), rep(base_pos))
    return {k: (v.reshape((S, P) + v.shape[1:]) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def evaluate(topo, capsules, pairs, floating, q, rpy, base_pos, ncand, sample, scale=None, pose_sample=None):
    """The contract of fbr_capsule_distance_gradients: q (C * T, n) [, rpy, base_pos], sample / scale / pose_sample (C, P) -> item_gradients'
    arrays as (C, P[, n]); an item with sample -1 has dist 1e10 and a zero row."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    C, P = int(ncand), pairs.shape[0]
    T = q.shape[0] // C
    sample = np.asarray(sample).reshape(C, P)
    pose = sample if pose_sample is None else np.where(np.asarray(pose_sample).reshape(C, P) < 0, sample, np.asarray(pose_sample).reshape(C, P))
    sc = np.ones((C, P)) if scale is None else np.asarray(scale, dtype=np.float64).reshape(C, P)
    base = (np.arange(C) * T)[:, None]
    rq = (base + np.maximum(sample, 0)).reshape(-1)
    rp = (base + np.maximum(pose, 0)).reshape(-1)
    out = item_gradients(topo, capsules, np.tile(pairs, (C, 1)), q[rq] * sc.reshape(-1, 1), floating, None if rpy is None else rpy[rp],
                         None if base_pos is None else base_pos[rp])
    out = {k: (v.reshape((C, P) + v.shape[1:]) if isinstance(v, np.ndarray) else v) for k, v in out.items()}
    none = sample < 0
    out["dist"] = np.where(none, cr.NONE, out["dist"])
    out["grad"] = np.where(none[..., None], 0.0, out["grad"])
    return out


def gradient_tolerance(ref):
    """per item: 1e-12 max(1, world scale) parameter_condition -- the distance tolerance of the project times the amplification of s and t,
    on which the gradient (unlike the distance) depends to first order"""
    return 1e-12 * ref["scale"] * ref["cond"]


def position_chain(wf, q_range, A, B, sample, scale, grad_q, freq, dtype=np.float64):
    """ONE candidate: A, B (n, nh), q_range (n,) or None, sample (R,) int, scale (R,) or None, grad_q (R, n) -> (R, 1 + 2 n + 2 n nh) in the
    layout of fbr_fourier_gradient: scale * sum_d grad_q[d] dq_d/dp at t = sample / freq; rows with sample < 0 are zero."""
    n, nh = np.asarray(A).shape
    sample = np.asarray(sample)
    R = sample.shape[0]
    t = np.maximum(sample, 0).astype(dtype) / dtype(freq)
    sc = np.ones(R, dtype=dtype) if scale is None else np.asarray(scale, dtype=dtype)
    out = np.zeros((R, 1 + 2 * n + 2 * n * nh), dtype=dtype)
    g = np.asarray(grad_q, dtype=dtype)
    for j in range(n):
        J = frest.series_jacobian(wf, None if q_range is None else q_range[j], A[j], B[j], t, dtype)[0]  # (R, K): the position's rows
        idx = np.concatenate([[0, 1 + j, 1 + n + j], 1 + 2 * n + j * nh + np.arange(nh), 1 + 2 * n + n * nh + j * nh + np.arange(nh)])
        out[:, idx] += (sc * g[:, j])[:, None] * J
    out[sample < 0] = 0
    return out
