"""An independent NumPy restatement of the capsule collision distances (the reference's excitation/capsule.py capsule_distance and the
collision block of excitation/trajectoryOptimizer.py objectiveFunc), vectorised over samples and pairs -- what the tests hold the
HIP-free text of csrc/fbr_capsule.h and the device against.  Link poses come from tests/np_dynamics.world_kinematics: no code shared with
the kernels."""
import numpy as np

from np_dynamics import rpy_R, world_kinematics

EPSILON = 1e-10
NONE = 1e10
# branch codes of segment_distance: the case, times 3, plus what happened to t (general case only)
BOTH_POINTS, A_POINT, B_POINT, GENERAL, PARALLEL = 0, 1, 2, 3, 4
T_INSIDE, T_BELOW, T_ABOVE = 0, 1, 2
BAND = 1e-6  # an evaluation is "on a threshold" when a, e or a e - b^2 lies within this (relative) of EPSILON


def _dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def segment_distance(a0, a1, b0, b1):
    """(..., 3) end points -> dict dist, s, t, branch, near (all (...)): Ericson's closest points of two segments with the reference's
    thresholds; ``near``: a decision quantity of this evaluation lies within BAND of its threshold."""
    a0, a1, b0, b1 = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (a0, a1, b0, b1)))
    d1, d2, r = a1 - a0, b1 - b0, a0 - b0
    a, e, f = _dot(d1, d1), _dot(d2, d2), _dot(d2, r)
    c, b = _dot(d1, r), _dot(d1, d2)
    denom = a * e - b * b
    pa, pb = a <= EPSILON, e <= EPSILON
    gen = ~pa & ~pb
    with np.errstate(all="ignore"):
        s_line = np.where(denom > EPSILON, np.clip((b * f - c * e) / denom, 0.0, 1.0), 0.0)
        t_line = (b * s_line + f) / e
        below, above = gen & (t_line < 0.0), gen & (t_line > 1.0)
        s_gen = np.where(below, np.clip(-c / a, 0.0, 1.0), np.where(above, np.clip((b - c) / a, 0.0, 1.0), s_line))
        t_gen = np.where(below, 0.0, np.where(above, 1.0, t_line))
        s = np.where(pa, 0.0, np.where(pb, np.clip(-c / a, 0.0, 1.0), s_gen))
        t = np.where(pb, 0.0, np.where(pa, np.clip(f / e, 0.0, 1.0), t_gen))
    diff = (a0 + s[..., None] * d1) - (b0 + t[..., None] * d2)
    dist = np.sqrt(_dot(diff, diff))
    case = np.where(pa & pb, BOTH_POINTS, np.where(pa, A_POINT, np.where(pb, B_POINT, np.where(denom > EPSILON, GENERAL, PARALLEL))))
    tcase = np.where(below, T_BELOW, np.where(above, T_ABOVE, T_INSIDE))
    on = lambda x: np.abs(x - EPSILON) <= BAND * EPSILON  # noqa: E731
    near = on(a) | on(e) | (gen & on(denom))
    return {"dist": dist, "s": s, "t": t, "branch": case * 3 + tcase, "near": near}


def parameter_condition(a0, a1, b0, b1):
    """How much the closest-point parameters s, t amplify rounding in the dot products they are quotients of: the magnitude of the
    numerators' terms, (|d1| + |d2|) (|r| + |d1| + |d2|), over the smallest divisor the evaluation uses (a, e, or (a e - b^2) / max(a, e)
    when the segments are not parallel).  The reference forms its dot products with BLAS (fused multiply-adds, another summation order than
    the left-to-right sums here), so its s and t agree with any other evaluation to rounding times this number only; the DISTANCE does not
    amplify (it is stationary in s and t, or clamped)."""
    d1, d2, r = a1 - a0, b1 - b0, a0 - b0
    n = lambda x: np.sqrt(_dot(x, x))  # noqa: E731
    a, e, b = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2)
    den = a * e - b * b
    pa, pb = a <= EPSILON, e <= EPSILON
    with np.errstate(all="ignore"):
        inv = np.maximum(np.where(pa, 0.0, 1.0 / a), np.where(pb, 0.0, 1.0 / e))
        inv = np.maximum(inv, np.where(~pa & ~pb & (den > EPSILON), np.maximum(a, e) / den, 0.0))
    return np.maximum(1.0, (n(d1) + n(d2)) * (n(r) + n(d1) + n(d2)) * inv)


def capsule_world(topo, capsules, q, floating=False, rpy=None, base_pos=None):
    """World end points (S, ncaps, 6) of ``capsules`` [(link index, p0, p1, radius)] at joint positions q (S, n); floating base:
    world_T_base = (RPY(rpy)^T, base_pos), the reference's setCollisionRobotState."""
    q = np.asarray(q, dtype=np.float64)
    S = q.shape[0]
    z = np.zeros((S, 3))
    if floating and rpy is not None:
        R = np.transpose(rpy_R(np.asarray(rpy, dtype=np.float64)), (0, 2, 1))
        pb = z if base_pos is None else np.asarray(base_pos, dtype=np.float64)
    else:
        R, pb = np.tile(np.eye(3), (S, 1, 1)), z
    k = world_kinematics(topo, q, 0 * q, 0 * q, R, z, z, z, z, p_b=pb)
    ep = np.empty((S, len(capsules), 6))
    for i, (l, p0, p1, _) in enumerate(capsules):
        ep[:, i, :3] = np.einsum("sij,j->si", k["R"][l], np.asarray(p0, dtype=np.float64)) + k["p"][l]
        ep[:, i, 3:] = np.einsum("sij,j->si", k["R"][l], np.asarray(p1, dtype=np.float64)) + k["p"][l]
    return ep


def capsule_distances(ep, capsules, pairs):
    """dict of (S, P) arrays (segment_distance's, ``dist`` minus the two radii) for world end points ep (S, ncaps, 6)."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    rad = np.array([c[3] for c in capsules], dtype=np.float64)
    A, B = ep[:, pairs[:, 0]], ep[:, pairs[:, 1]]
    out = segment_distance(A[..., :3], A[..., 3:], B[..., :3], B[..., 3:])
    out["dist"] = out["dist"] - rad[pairs[:, 0]] - rad[pairs[:, 1]]
    return out


def candidate_minimum(dist, ncand, step):
    """dist (C * T, P) -> (val (C, P), idx (C, P) int64): per candidate, the minimum over the samples 0, step, ... walked upwards with a
    strict < from 1e10 -- the first sample wins a tie, a NaN never wins, (1e10, -1) when no sample wins."""
    S, P = dist.shape
    T = S // ncand
    d = dist.reshape(ncand, T, P)[:, ::step]
    with np.errstate(invalid="ignore"):
        m = np.where(d < NONE, d, np.inf)
    k = np.argmin(m, axis=1)
    v = np.take_along_axis(m, k[:, None], axis=1)[:, 0]
    won = np.isfinite(v) | (v == -np.inf)
    return np.where(won, v, NONE), np.where(won, k * step, -1).astype(np.int64)


def world_scale(ep):
    """largest |world coordinate| of a case (the tolerance of the device comparison scales with it), NaN poses aside"""
    return float(np.nanmax(np.abs(ep))) if np.isfinite(ep).any() else 1.0


# ---- capsule sets the tests share ---------------------------------------------------------------------------------------------------
def synthetic_capsules(topo, radius=0.03):
    """a capsule on every link: from the link's origin to its first child's origin (a leaf: 5 cm along z); many are spheres or very
    short -- [(link index, p0, p1, radius)]"""
    L = topo.num_links
    rp = np.asarray(topo.rest_p, dtype=np.float64).reshape(L, 3)
    caps = []
    for l in range(L):
        ch = [c for c in range(L) if topo.parent[c] == l]
        caps.append((l, np.zeros(3), rp[ch[0]].copy() if ch else np.array([0.0, 0.0, 0.05]), radius))
    return caps


def non_neighbour_pairs(topo, capsules):
    """every pair of capsules whose links are not parent and child, sorted by the first capsule"""
    out = []
    for i in range(len(capsules)):
        for j in range(i + 1, len(capsules)):
            li, lj = capsules[i][0], capsules[j][0]
            if li != lj and topo.parent[li] != lj and topo.parent[lj] != li:
                out.append((i, j))
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def fitted_capsules(golden_npz, robot, topo, tag=""):
    """the capsules the reference fitted to ``robot`` (tests/golden/ref_capsules.npz), on the links the topology kept"""
    z = golden_npz
    names = list(topo.link_names)
    return [(names.index(str(n)), z[f"fit_{robot}{tag}_p0"][i], z[f"fit_{robot}{tag}_p1"][i], float(z[f"fit_{robot}{tag}_radius"][i]))
            for i, n in enumerate(z[f"fit_{robot}{tag}_links"]) if str(n) in names]


def device_case(topo, capsules, pairs, st, ncand, step, floating, base_pos=None):
    """what the device has to return for a case -- (val, idx, dist (S, P), scale) -- after asserting that no evaluation of the case sits on a
    branch threshold (nothing is left out of a comparison)"""
    ep = capsule_world(topo, capsules, st["q"], floating, st.get("rpy"), base_pos)
    d = capsule_distances(ep, capsules, pairs)
    assert int(d["near"].sum()) == 0, "an evaluation of this seed lies on a branch threshold: change the seed"
    val, idx = candidate_minimum(d["dist"], ncand, step)
    return val, idx, d["dist"], max(1.0, world_scale(ep))


def assert_device_matches(got_val, got_idx, val, idx, dist, ncand, scale, why=""):
    """|delta dist| <= 1e-12 max(1, largest |world coordinate|); an index may differ only where the restatement's own distance at the
    device's index is within that tolerance of its minimum.  Returns the largest difference seen."""
    tol = 1e-12 * scale
    none = idx < 0
    assert np.array_equal(got_idx < 0, none), (why, "pairs without a winning sample")
    assert np.all(got_val[none] == NONE), why
    err = float(np.abs(got_val[~none] - val[~none]).max()) if (~none).any() else 0.0
    assert err <= tol, (why, err, tol)
    diff = (got_idx != idx) & ~none
    if diff.any():
        T = dist.shape[0] // ncand
        d3 = dist.reshape(ncand, T, -1)
        c, k = np.nonzero(diff)
        assert np.all(np.abs(d3[c, got_idx[c, k], k] - val[c, k]) <= tol), (why, "index differs beyond rounding")
    return err
