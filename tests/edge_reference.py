"""Edge batches and their long-double reference (test helper, not shipped).

The reference is tests/np_dynamics.py's world-frame kinematics run in ``np.longdouble`` (64-bit mantissa: rounding 5e-20 against
double's 1e-16), with the link wrenches written about the link ORIGIN so that they are linear in the ten standard parameters
``[m, m c, I_origin]``: the regressor is then the inverse dynamics of the unit parameter vectors, link by link.  No code or convention is
shared with oracle/fbr_oracle.c (body-frame spatial algebra) or the kernels (base-frame composite regressor).

The batches hold equally sized classes of states, CLASS_SIZE samples each and class after class, so that a 64-sample wave and an image of
the Gram pass straddle class boundaries (nine classes, 216 samples, leave a partial wave as well; eight give 192, three whole waves whose
boundaries at 64 and 128 cut classes).  Every comparison made with them is scaled per sample (or per class): a fast sample cannot loosen
the bar of a resting one.
"""
from __future__ import annotations

import functools

import numpy as np

import capsule_restatement as cr
import np_dynamics as nd
from common import load_topo, random_states, random_topology

LD = np.longdouble
CLASS_SIZE = 24
BAR = 1e-11            # the project's own parity bar, applied per sample / per class
ORACLE_CLEAN = 1e-12   # a class whose double oracle stays below this keeps BAR; above it the bar is 8 x the oracle's ratio (ORACLE_RATIO)
REPLACED = 70          # the sample the neighbour tests replace: inside the third class, two samples before a class boundary

# (key, robot or None for the random tree, floating, friction, Stribeck velocity); friction is symmetric everywhere
EDGE_CONFIGS = [
    ("threeLinks-fb", "threeLinks", 1, 0, 0.0),
    ("kuka-fric-st0.05", "kuka_lwr4", 0, 1, 0.05),
    ("walkman_left_arm-fb-fric", "walkman_left_arm", 1, 1, 0.0),
    ("tree12-fb", None, 1, 0, 0.0),
]
CONFIG_KEYS = [c[0] for c in EDGE_CONFIGS]

# Worst per-sample ratio max|Y_o[s] - Y_ref[s]| / max|Y_ref[s]| of the DOUBLE oracle (regressor, inverse dynamics, contact torques) above
# ORACLE_CLEAN, by (configuration, class), as tests/test_edge_reference.py measures and pins it ("Parity at state edges", lists every figure).  That
# is conditioning of the state, not a fault: the device bar of such a class is 8 x this number -- one order of magnitude for another order
# of operations -- and never comes from the kernels.  Empty: the oracle stays below 1e-12 in every class.
ORACLE_RATIO: dict = {}


def class_bar(key: str, cls: str) -> float:
    r = ORACLE_RATIO.get((key, cls), 0.0)
    return 8.0 * r if r > ORACLE_CLEAN else BAR


@functools.lru_cache(maxsize=None)
def config(key: str):
    """(topology, floating, friction, stribeck) of an edge configuration"""
    _, name, fl, fr, strb = EDGE_CONFIGS[CONFIG_KEYS.index(key)]
    if name is None:
        topo = random_topology(np.random.default_rng(1212), 12, p_fixed=0.2, p_prismatic=0.3)
        assert 2 in topo.joint_type and 0 in topo.joint_type[1:] and topo.num_dofs >= 6
    else:
        topo = load_topo(name)
    return topo, bool(fl), bool(fr), float(strb)


# ------------------------------------------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------------------------------------------
def _pm(rng, shape, scale):
    return (rng.random(shape) * 2 - 1) * scale


def edge_batch(key: str, seed: int = 5):
    """-> (states, class names): states of len(names) * CLASS_SIZE samples, with ``sign`` and ``vel_sign`` for a friction model."""
    topo, floating, friction, stribeck = config(key)
    rng = np.random.default_rng([seed, CONFIG_KEYS.index(key)])
    n, T = topo.num_dofs, CLASS_SIZE
    prismatic = np.zeros(n, dtype=bool)
    for l, d in enumerate(topo.dof_index):
        if d >= 0 and topo.joint_type[l] == 2:
            prismatic[d] = True
    classes = []

    def ordinary():
        return random_states(topo, T, rng, floating)

    classes.append(("ordinary", ordinary()))

    st = ordinary()
    st["dq"][:] = 0.0
    st["ddq"][:] = 0.0
    if floating:
        st["base_vel"][:] = 0.0
        st["base_acc"][:] = 0.0
    classes.append(("rest", st))

    st = ordinary()
    st["q"] = rng.choice(np.array([0.0, -0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi]), size=(T, n))
    st["q"][0, :] = -0.0  # (one sample with every joint at -0.0, one with every joint at pi)
    st["q"][1, :] = np.pi
    classes.append(("exact", st))

    st = ordinary()
    for k in ("q", "dq", "ddq"):
        st[k] = _pm(rng, (T, n), 1e-8)
        st[k][2, :] = [(5e-324, -1e-310, 1e-310, -5e-324)[j % 4] for j in range(n)]
    classes.append(("tiny", st))

    st = ordinary()
    turns = rng.integers(-100000, 100001, size=(T, n)).astype(np.float64)
    turns[0, :] = 100000.0
    turns[1, :] = -100000.0
    st["q"] = np.where(prismatic[None], np.where(rng.random((T, n)) < 0.5, -50.0, 50.0), 2 * np.pi * turns + st["q"])
    classes.append(("multiturn", st))

    st = ordinary()
    st["dq"] = _pm(rng, (T, n), 1e3)
    classes.append(("fast", st))

    st = ordinary()
    st["ddq"] = _pm(rng, (T, n), 1e5)
    classes.append(("hardacc", st))

    if floating:
        st = ordinary()
        st["rpy"] = -_pm(rng, (T, 3), np.pi)  # (-pi, pi]
        h = np.pi / 2
        st["rpy"][:12, 1] = [h, -h, h, -h, h, -h, h - 1e-9, -(h - 1e-9), h - 1e-9, -(h - 1e-9), h - 1e-9, -(h - 1e-9)]
        st["rpy"][12:, 1] = _pm(rng, T - 12, h)
        st["base_vel"] = _pm(rng, (T, 6), np.pi)
        st["base_acc"] = _pm(rng, (T, 6), np.pi)
        classes.append(("attitude", st))

    if friction:
        for _, s in classes:
            s["sign"] = np.tanh(s["dq"] / 0.02)
            s["vel_sign"] = 0.9 * s["dq"]
        st = ordinary()
        # dq exactly 0 (both zeros) and +-1e-12; the Stribeck exponential exp(-|dq| / v_s) underflows in double from |dq| / v_s > 745
        v = np.array([0.0, -0.0, 1e-12, -1e-12, 40.0, -40.0, 1e3, -1e3])
        st["dq"] = rng.choice(v, size=(T, n))
        st["dq"][:8] = np.broadcast_to(v[:, None], (8, n))
        st["sign"] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0]), size=(T, n))
        st["sign"][8:12] = np.broadcast_to(np.array([0.0, -0.0, 1.0, -1.0])[:, None], (4, n))
        st["vel_sign"] = st["dq"].copy()
        classes.append(("friction", st))

    names = [c for c, _ in classes]
    keys = classes[0][1].keys()
    out = {k: np.ascontiguousarray(np.concatenate([s[k] for _, s in classes])) for k in keys}
    return out, names


def class_slices(names):
    return {c: slice(i * CLASS_SIZE, (i + 1) * CLASS_SIZE) for i, c in enumerate(names)}


def engine_states(st):
    """the keys Engine / OracleModel take as states (vel_sign is an argument of its own)"""
    return {k: v for k, v in st.items() if k != "vel_sign"}


def sample_states(st, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}


def with_sample(st, s, other, o):
    """copy of st with sample s replaced by sample o of ``other``"""
    out = {k: v.copy() for k, v in st.items()}
    for k in out:
        out[k][s] = other[k][o]
    return out


def nan_state(st, s):
    """copy of st whose sample s has q, dq and rpy (and what follows from dq: sign, vel_sign) all NaN"""
    out = {k: v.copy() for k, v in st.items()}
    for k in ("q", "dq", "rpy", "sign", "vel_sign"):
        if k in out:
            out[k][s] = np.nan
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the long-double reference
# ------------------------------------------------------------------------------------------------------------------------------------
def _kinematics(topo, st, floating, need_vel=True):
    S = st["q"].shape[0]
    q = np.asarray(st["q"], dtype=LD)
    zq = np.zeros_like(q)
    dq = np.asarray(st["dq"], dtype=LD) if need_vel else zq
    ddq = np.asarray(st["ddq"], dtype=LD) if need_vel else zq
    z = np.zeros((S, 3), dtype=LD)
    if floating:
        R_wb = np.transpose(nd.rpy_R(st["rpy"], LD), (0, 2, 1))
        if need_vel:
            bv, ba = np.asarray(st["base_vel"], dtype=LD), np.asarray(st["base_acc"], dtype=LD)
            return nd.world_kinematics(topo, q, dq, ddq, R_wb, bv[:, :3], bv[:, 3:], ba[:, :3], ba[:, 3:], dtype=LD)
    else:
        R_wb = np.tile(np.eye(3, dtype=LD), (S, 1, 1))
    return nd.world_kinematics(topo, q, dq, ddq, R_wb, z, z, z, z, dtype=LD)


def _link_wrench(k, l, P, g):
    """Net force F and net moment N about the ORIGIN of link l, world axes, (K, S, 3) each, for K parameter vectors P (K, 10) of that link:
    F = m (a - g) + dw x h + w x (w x h),  N = I dw + w x I w + h x (a - g),  h = R (m c), I = R I_origin R^T -- linear in P."""
    R, w, dw = k["R"][l], k["w"][l][None], k["dw"][l][None]
    ag = (k["a"][l] - g[None])[None]
    h = np.einsum("sij,kj->ksi", R, P[:, 1:4])
    Io = np.empty((P.shape[0], 3, 3), dtype=LD)
    for (i, j), c in {(0, 0): 4, (0, 1): 5, (0, 2): 6, (1, 1): 7, (1, 2): 8, (2, 2): 9}.items():
        Io[:, i, j] = Io[:, j, i] = P[:, c]
    Iw = np.einsum("sij,kjm,snm->ksin", R, Io, R)
    F = P[:, 0, None, None] * ag + np.cross(dw, h) + np.cross(w, np.cross(w, h))
    N = np.einsum("ksij,sj->ksi", Iw, dw[0]) + np.cross(w, np.einsum("ksij,sj->ksi", Iw, w[0])) + np.cross(h, ag)
    return F, N


def _project(topo, k, floating, l, p_at, F, N):
    """Generalised forces (K, S, rows) of a wrench (F, N about the point p_at (S, 3)) that acts on link l: the base wrench about the base
    origin in world axes, and along every joint between l and the base the moment about / the force along its axis."""
    n, fb = topo.num_dofs, 6 if floating else 0
    axis = np.asarray(topo.axis, dtype=LD)
    tau = np.zeros(F.shape[:2] + (n + fb,), dtype=LD)
    if floating:
        tau[..., 0:3] = F
        tau[..., 3:6] = N + np.cross(p_at[None], F)
    while topo.parent[l] >= 0:
        d = topo.dof_index[l]
        if d >= 0:
            sw = np.einsum("sij,j->si", k["R"][l], axis[l])[None]
            if topo.joint_type[l] == 2:
                tau[..., fb + d] = np.sum(sw * F, axis=-1)
            else:
                tau[..., fb + d] = np.sum(sw * (N + np.cross((p_at - k["p"][l])[None], F)), axis=-1)
        l = topo.parent[l]
    return tau


def _friction_start(topo):
    return 10 * topo.num_links


def regressor_ld(key: str, st, gravity=(0.0, 0.0, -9.81), friction_symmetric=True, gravity_only=False):
    """Y_ref (S, rows, P) in long double: the inertial block by linearity (column 10 l + c = inverse dynamics of the unit parameter e_c of
    link l), then the friction columns from their closed forms -- Coulomb: the sign series; viscous: dq, or max(dq, 0) | min(dq, 0) when
    asymmetric; offset: 1; Stribeck: exp(-|dq| / v_s) sgn(dq).  gravity_only keeps [m, m c] of every link and the Coulomb block, by
    indexing."""
    topo, floating, friction, stribeck = config(key)
    S, n, L = st["q"].shape[0], topo.num_dofs, topo.num_links
    fb = 6 if floating else 0
    k = _kinematics(topo, st, floating)
    g = np.asarray(gravity, dtype=LD)
    E = np.eye(10, dtype=LD)
    blocks = []
    for l in range(L):
        F, N = _link_wrench(k, l, E, g)
        blocks.append(np.transpose(_project(topo, k, floating, l, k["p"][l], F, N), (1, 2, 0)))  # (S, rows, 10)
    if friction:
        dq = np.asarray(st["dq"], dtype=LD)
        dg = np.zeros((n + fb, n), dtype=LD)
        dg[fb:, :] = np.eye(n, dtype=LD)
        col = lambda v: dg[None] * v[:, None, :]  # noqa: E731  (S, rows, n): v[s, j] in row fb + j, column j
        blocks.append(col(np.asarray(st["sign"], dtype=LD)))
        if not gravity_only:
            if friction_symmetric:
                blocks.append(col(dq))
            else:
                blocks += [col(np.where(dq < 0, LD(0), dq)), col(np.where(dq > 0, LD(0), dq))]
            blocks.append(col(np.ones_like(dq)))
            if stribeck > 0:
                blocks.append(col(np.exp(-np.abs(dq) / LD(stribeck)) * np.sign(dq)))
    Y = np.concatenate(blocks, axis=2)
    if gravity_only:
        keep = [10 * l + c for l in range(L) for c in range(4)] + list(range(10 * L, Y.shape[2]))
        Y = Y[:, :, keep]
    return Y


def torques_ld(key: str, st, x_std, gravity=(0.0, 0.0, -9.81)):
    """Generalised torques (S, rows) in long double for the standard vector x_std = [10 L inertial | Fc | Fv | offset | Fs] (the symmetric
    friction layout): rigid-body part + sign Fc + Fv dq + offset + Fs exp(-|vel_sign| / v_s) sgn(sign)."""
    topo, floating, friction, stribeck = config(key)
    n, L = topo.num_dofs, topo.num_links
    fb = 6 if floating else 0
    k = _kinematics(topo, st, floating)
    g = np.asarray(gravity, dtype=LD)
    X = np.asarray(x_std, dtype=LD)
    tau = 0
    for l in range(L):
        F, N = _link_wrench(k, l, X[None, 10 * l:10 * l + 10], g)
        tau = tau + _project(topo, k, floating, l, k["p"][l], F, N)[0]
    if friction:
        f0 = _friction_start(topo)
        sg, dq = np.asarray(st["sign"], dtype=LD), np.asarray(st["dq"], dtype=LD)
        t = sg * X[f0:f0 + n] + X[f0 + n:f0 + 2 * n] * dq + X[f0 + 2 * n:f0 + 3 * n]
        if stribeck > 0:
            t = t + X[f0 + 3 * n:f0 + 4 * n] * np.exp(-np.abs(np.asarray(st["vel_sign"], dtype=LD)) / LD(stribeck)) * np.sign(sg)
        tau[:, fb:] += t
    return tau


def contact_frame(key: str):
    """the link the contact tests push on: the deepest link of the tree (the last one on ties)"""
    topo = config(key)[0]
    depth = [0] * topo.num_links
    for l in topo.traversal():
        if topo.parent[l] >= 0:
            depth[l] = depth[topo.parent[l]] + 1
    return topo.link_names[max(range(topo.num_links), key=lambda l: (depth[l], l))]


def contact_torques_ld(key: str, st, frame: str, wrench):
    """J^T w (S, rows) in long double for a wrench [force; torque] in world axes at the origin of link ``frame``."""
    topo, floating, _, _ = config(key)
    l = topo.link_names.index(frame)
    k = _kinematics(topo, st, floating, need_vel=False)
    w = np.asarray(wrench, dtype=LD)
    return _project(topo, k, floating, l, k["p"][l], w[None, :, :3], w[None, :, 3:])[0]


def per_sample_ratio(got, ref):
    """max|got[s] - ref[s]| / max|ref[s]| per sample, in long double; got / ref (S, ...).  A sample whose reference is all zero counts
    0 when got is zero too, inf otherwise."""
    S = ref.shape[0]
    d = np.abs(np.asarray(got, dtype=LD).reshape(S, -1) - ref.reshape(S, -1)).max(axis=1)
    m = np.abs(ref.reshape(S, -1)).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m > 0, d / np.where(m > 0, m, 1), np.where(d > 0, np.inf, 0.0)).astype(np.float64)


def worst_by_class(ratio, names):
    return {c: float(ratio[sl].max()) for c, sl in class_slices(names).items()}


@functools.lru_cache(maxsize=None)
def reference(key: str):
    """Everything the tests of one configuration compare against, computed once and shared (treat it as read-only): the edge batch, its
    classes, the parameter vectors, the wrench, and the long-double regressor, torques, predictions and contact torques."""
    topo, floating, friction, stribeck = config(key)
    st, names = edge_batch(key)
    S = st["q"].shape[0]
    rng = np.random.default_rng([77, CONFIG_KEYS.index(key)])
    Y = regressor_ld(key, st)
    P = Y.shape[2]
    x_std = rng.standard_normal(P)      # entries of both signs: the torques are linear in it, physical consistency is not needed
    x_pred = rng.standard_normal(P)
    wrench = rng.standard_normal((S, 6))
    frame = contact_frame(key)
    ref = {"st": st, "names": names, "S": S, "P": P, "rows": Y.shape[1], "x_std": x_std, "x_pred": x_pred, "wrench": wrench, "frame": frame,
           "Y": Y, "tau": torques_ld(key, st, x_std), "pred": np.einsum("srp,p->sr", Y, np.asarray(x_pred, dtype=LD)),
           "contact": contact_torques_ld(key, st, frame, wrench)}
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    for v in st.values():
        v.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------------------------------------------------
# capsule poses
# ------------------------------------------------------------------------------------------------------------------------------------
CAPSULE_CLASSES = ("exact", "multiturn", "attitude")
CAPSULE_KEYS = ("threeLinks-fb", "tree12-fb")


def capsule_case(key):
    """-> (topology, capsules, pairs, states of the three classes, restatement distances (3 T, pairs), per-sample bar (3 T,)).  One capsule
    per moving link -- with a floating base every link moves; fixed links ride on their parent and get none -- between two points drawn
    for it, both off the joint axis (an end point on the axis does not move with the joint: different poses, the same distance), and all
    pairs.  Bar: 1e-11 x the largest distance of a capsule end point from the base origin in that sample."""
    topo, floating, _, _ = config(key)
    ref = reference(key)
    rng = np.random.default_rng([80, CONFIG_KEYS.index(key)])
    caps = [(l, rng.standard_normal(3) * 0.1, rng.standard_normal(3) * 0.2, 0.02) for l in range(topo.num_links)
            if topo.parent[l] < 0 or topo.dof_index[l] >= 0]
    pairs = np.array([(i, j) for i in range(len(caps)) for j in range(i + 1, len(caps))], dtype=np.int32)
    sl = class_slices(ref["names"])
    st = {k: np.concatenate([ref["st"][k][sl[c]] for c in CAPSULE_CLASSES]) for k in ("q", "rpy")}
    ep = cr.capsule_world(topo, caps, st["q"], floating, st["rpy"])
    d = cr.capsule_distances(ep, caps, pairs)
    assert int(d["near"].sum()) == 0, "an evaluation lies on a branch threshold: change the seed"
    reach = np.sqrt((ep.reshape(ep.shape[0], -1, 3) ** 2).sum(axis=2)).max(axis=1)
    return topo, caps, pairs, st, d["dist"], BAR * reach


def undecided_pairs(dist, bar):
    """(3, pairs) bool: the restatement's two best samples of the class lie within the bar of each other -- the winner is rounding's"""
    d3 = np.sort(dist.reshape(len(CAPSULE_CLASSES), CLASS_SIZE, -1), axis=1)
    return (d3[:, 1] - d3[:, 0]) <= bar.reshape(len(CAPSULE_CLASSES), CLASS_SIZE).max(axis=1)[:, None]
