"""CPU restatement of the reference's ``simulate_suspended_base_motion`` (excitation/suspendedDynamics.py), twice (test helper, not shipped).

(a) ``simulate_direct``: the reference's loop step by step, vectorised over the candidates.  At every step the moment about the attachment
    origin O and its three angular-acceleration columns come from a full world-frame Newton-Euler on ``np_dynamics.world_kinematics`` -- the
    base link is given the state that holds the attachment frame at O (asserted at every step); no records, no probes.  ``dtype`` =
    ``np.longdouble`` evaluates everything in extended precision: the yardstick of the device tests.
(b) ``sample_records`` + ``simulate_from_records``: the 39-double record per sample and the O(1) step the device kernels implement.

Record layout (everything in the attachment link's axes, about its origin O): I (xx xy xz yy yz zz) | B (3 x 3 row-major) | c0 | mc |
R (3 x 3), p of the base link relative to the attachment frame | its twist [lin; ang] relative to that frame."""
from __future__ import annotations

import numpy as np

from np_dynamics import link_inertials, rpy_R, world_kinematics

EQ_MAX_ITER, EQ_TOL, EQ_STEP, EQ_CLIP_DEG, MAX_SWING_DEG, BOUNCE = 200, 0.01, 1.0 / 700.0, 30.0, 25.0, -0.3
REC = 39
OFF_I, OFF_B, OFF_C0, OFF_MC, OFF_R, OFF_P, OFF_V = 0, 6, 15, 18, 21, 30, 33


def _mv(A, x):
    return np.einsum("...ij,...j->...i", A, x)


def _mtv(A, x):
    return np.einsum("...ji,...j->...i", A, x)


def _solve3(M, b):
    """x = M^-1 b, batched 3 x 3, by cofactors (any dtype: np.linalg.solve has no extended precision)"""
    c = np.empty_like(M)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            s = [k for k in range(3) if k != j]
            c[..., i, j] = (-1) ** (i + j) * (M[..., r[0], s[0]] * M[..., r[1], s[1]] - M[..., r[0], s[1]] * M[..., r[1], s[0]])
    det = (M[..., 0, :] * c[..., 0, :]).sum(-1)
    return np.einsum("...ji,...j->...i", c, b) / det[..., None]


def rest_kinematics(topo, att, q, dq, ddq, dtype=np.float64):
    """the attachment link relative to the base link, in the base link's axes: kinematics with the base at rest at the origin"""
    S = q.shape[0]
    z = np.zeros((S, 3), dtype=dtype)
    k = world_kinematics(topo, q, dq, ddq, np.tile(np.eye(3, dtype=dtype), (S, 1, 1)), z, z, z, z, dtype=dtype)
    return {key: k[key][att] for key in k}


def base_state(rest, R, om, al):
    """State of the base link that holds the attachment frame at O with world orientation R (S, 3, 3), angular velocity om, angular
    acceleration al (world axes) and its origin at rest: (R_wb, p_b, v_b, w_b, a_b, dw_b)."""
    Rwb = R @ np.swapaxes(rest["R"], -1, -2)
    r, vrel, wrel, arel, dwrel = (_mv(Rwb, rest[key]) for key in ("p", "v", "w", "a", "dw"))
    wb = om - wrel
    dwb = al - np.cross(wb, wrel) - dwrel
    vb = -(np.cross(wb, r) + vrel)
    ab = -(np.cross(dwb, r) + np.cross(wb, np.cross(wb, r)) + 2 * np.cross(wb, vrel) + arel)
    return Rwb, -r, vb, wb, ab, dwb


def direct_moment(topo, att, q, dq, ddq, R, om, al, gravity, dtype=np.float64, rest=None, check=True, inert=None):
    """Moment about O (world axes) that inverse dynamics asks for with the attachment frame at O, orientation R, angular velocity om,
    angular acceleration al: world-frame Newton-Euler about every link's centre of mass.  Returns (moment (S, 3), kinematics)."""
    q, dq, ddq = (np.asarray(x, dtype=dtype) for x in (q, dq, ddq))
    if rest is None:
        rest = rest_kinematics(topo, att, q, dq, ddq, dtype)
    Rwb, pb, vb, wb, ab, dwb = base_state(rest, R, om, al)
    k = world_kinematics(topo, q, dq, ddq, Rwb, vb, wb, ab, dwb, p_b=pb, dtype=dtype)
    if check:  # the attachment origin stays at O with zero velocity and acceleration, the frame turns as asked
        scale = 1.0 + max(float(np.abs(k["p"]).max()), float(np.abs(k["v"]).max()), float(np.abs(k["a"]).max()))
        tol = 1e-10 * scale
        assert np.abs(k["p"][att]).max() < tol and np.abs(k["v"][att]).max() < tol and np.abs(k["a"][att]).max() < tol
        assert np.abs(k["w"][att] - om).max() < tol and np.abs(k["dw"][att] - al).max() < tol
        assert np.abs(k["R"][att] - R).max() < 1e-12
    m, com, Ic = inert if inert is not None else link_inertials(topo, dtype)
    g = np.asarray(gravity, dtype=dtype)
    N = np.zeros(q.shape[:1] + (3,), dtype=dtype)
    for l in range(topo.num_links):
        Rl, w, dw = k["R"][l], k["w"][l], k["dw"][l]
        rc = _mv(Rl, com[l])
        ac = k["a"][l] + np.cross(dw, rc) + np.cross(w, np.cross(w, rc))
        F = m[l] * (ac - g[None])
        Iw = Rl @ Ic[l][None] @ np.swapaxes(Rl, -1, -2)
        N += _mv(Iw, dw) + np.cross(w, _mv(Iw, w)) + np.cross(k["p"][l] + rc, F)
    return N, k


def as_rpy(R):
    """iDynTree Rotation.asRPY, general branch: R = Rz(y) Ry(p) Rx(r)"""
    return np.stack([np.arctan2(R[..., 2, 1], R[..., 2, 2]), np.arcsin(-R[..., 2, 0]), np.arctan2(R[..., 1, 0], R[..., 0, 0])], axis=-1)


def rpy_rates(rpy, om):
    """angular_velocity_to_rpy_rates of excitation/simulationEffects.py as written, batched"""
    cr, sr, cp, sp = np.cos(rpy[:, 0]), np.sin(rpy[:, 0]), np.cos(rpy[:, 1]), np.sin(rpy[:, 1])
    z = np.zeros_like(cr)
    E = (1.0 / cp)[:, None, None] * np.stack([np.stack([cp, sr * sp, cr * sp], -1), np.stack([z, cr * cp, -sr * cp], -1), np.stack([z, sr, cr], -1)], -2)
    return _mv(E, om)


def _base_acc(vel, dt):
    C, T = vel.shape[:2]
    acc = np.zeros_like(vel)
    if T > 2:
        acc[:, 1:-1] = (vel[:, 2:] - vel[:, :-2]) / (2 * dt)
        acc[:, 0] = (vel[:, 1] - vel[:, 0]) / dt
        acc[:, -1] = (vel[:, -1] - vel[:, -2]) / dt
    return acc


def _integrate(rpy, om, al, dt, swing, stats):
    """one semi-implicit Euler step with the reference's soft clamp (in place); stats: per-candidate counters of the clamp path"""
    om += al * dt
    rpy += rpy_rates(rpy, om) * dt
    stats["margin"] = min(stats["margin"], float(np.abs(np.abs(rpy) - swing).min()))
    hi, lo = rpy > swing, rpy < -swing
    rev = (hi & (om > 0)) | (lo & (om < 0))
    rpy[hi] = swing
    rpy[lo] = -swing
    om[rev] *= BOUNCE
    cl = hi | lo
    stats["clamps"] += cl.sum(1)
    stats["reversals"] += rev.sum(1)
    stats["free_after_clamp"] += (stats["last_clamped"] & ~cl.any(1)).astype(np.int64)
    stats["last_clamped"] = cl.any(1)


def _new_stats(C):
    return {"clamps": np.zeros(C, dtype=np.int64), "reversals": np.zeros(C, dtype=np.int64), "free_after_clamp": np.zeros(C, dtype=np.int64),
            "last_clamped": np.zeros(C, dtype=bool), "margin": np.inf}


def _result(rpy_s, pos_s, vel_s, att_s, dt, iters, stats, C, T):
    info = np.stack([iters, stats["clamps"]], axis=1).astype(np.int64)
    flat = lambda a: a.reshape(C * T, -1)  # noqa: E731
    return {"rpy": flat(rpy_s), "base_position": flat(pos_s), "base_vel": flat(vel_s), "base_acc": flat(_base_acc(vel_s, dt)),
            "att_state": flat(att_s), "info": info, "stats": stats}


def simulate_direct(topo, att, q, dq, ddq, ncand, dt, damping, gravity=(0.0, 0.0, -9.81), dtype=np.float64):
    """Form (a).  q, dq, ddq (C * T, n): C equal candidates of T consecutive samples.  Returns the arrays of
    ``Engine.suspended_base_motion(..., with_info=True)`` in ``dtype`` plus ``stats`` (clamp-path counters and the smallest distance of an
    angle from +-25 degrees before clamping)."""
    C = int(ncand)
    T = q.shape[0] // C
    n = q.shape[1]
    Q, DQ, DDQ = (np.asarray(x, dtype=dtype).reshape(C, T, n) for x in (q, dq, ddq))
    inert = link_inertials(topo, dtype)
    base = int(np.flatnonzero(np.asarray(topo.parent) < 0)[0])
    eye4 = np.concatenate([np.zeros((1, 3), dtype=dtype), np.eye(3, dtype=dtype)])  # alpha = 0, e_x, e_y, e_z
    z3 = np.zeros((C, 3), dtype=dtype)
    eqlim, swing = dtype(np.deg2rad(EQ_CLIP_DEG)), dtype(np.deg2rad(MAX_SWING_DEG))
    # equilibrium at sample 0 with zero velocities; every candidate iterates until its own moment is below the tolerance
    rpy = np.zeros((C, 3), dtype=dtype)
    iters = np.full(C, EQ_MAX_ITER, dtype=np.int64)
    active = np.ones(C, dtype=bool)
    zq = np.zeros((C, n), dtype=dtype)
    rest0 = rest_kinematics(topo, att, Q[:, 0], zq, zq, dtype)
    for it in range(EQ_MAX_ITER):
        h, _ = direct_moment(topo, att, Q[:, 0], zq, zq, rpy_R(rpy, dtype), z3, z3, gravity, dtype, rest=rest0, inert=inert)
        done = active & (np.sqrt((h * h).sum(1)) < EQ_TOL)
        iters[done] = it + 1
        active &= ~done
        if not active.any():
            break
        step = np.clip(rpy - dtype(EQ_STEP) * h, -eqlim, eqlim)
        rpy = np.where(active[:, None], step, rpy)
    om = np.zeros((C, 3), dtype=dtype)
    rpy_s, pos_s, vel_s, att_s = (np.zeros((C, T, k), dtype=dtype) for k in (3, 3, 6, 6))
    stats = _new_stats(C)
    rep = lambda a: np.tile(a, (4,) + (1,) * (a.ndim - 1))  # noqa: E731
    for t in range(T):
        R = rpy_R(rpy, dtype)
        rest = rest_kinematics(topo, att, Q[:, t], DQ[:, t], DDQ[:, t], dtype)
        al4 = np.repeat(eye4, C, axis=0)
        N4, k = direct_moment(topo, att, rep(Q[:, t]), rep(DQ[:, t]), rep(DDQ[:, t]), rep(R), rep(om), al4, gravity, dtype,
                              rest={key: rep(v) for key, v in rest.items()}, inert=inert)
        N4 = N4.reshape(4, C, 3)
        Mbb = np.stack([N4[1 + i] - N4[0] for i in range(3)], axis=-1)  # columns: the moment per unit angular acceleration
        Meff = Mbb + dtype(damping) * dtype(dt) * np.eye(3, dtype=dtype)[None]
        rhs = -N4[0] - dtype(damping) * om
        al = np.linalg.solve(Meff, rhs[..., None])[..., 0] if dtype == np.float64 else _solve3(Meff, rhs)
        Rwb = k["R"][base][:C]
        rpy_s[:, t] = as_rpy(np.swapaxes(Rwb, -1, -2))
        pos_s[:, t] = k["p"][base][:C]
        vel_s[:, t, :3], vel_s[:, t, 3:] = k["v"][base][:C], k["w"][base][:C]
        att_s[:, t, :3], att_s[:, t, 3:] = rpy, om
        if t < T - 1:
            rpy, om = rpy.copy(), om.copy()
            _integrate(rpy, om, al, dtype(dt), swing, stats)
    return _result(rpy_s, pos_s, vel_s, att_s, dtype(dt), iters, stats, C, T)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) the record and the O(1) step
# ---------------------------------------------------------------------------------------------------------------------------------------
def sample_records(topo, att, q, dq, ddq, dtype=np.float64):
    """(S, 39) records.  I and mc: sums over the links; c0 and B: the direct moment at zero gravity with the attachment frame at
    orientation 1, angular acceleration 0 and angular velocity 0, e_x, e_y, e_z:  N(e_i) = c0 + B e_i + e_i x I e_i."""
    q, dq, ddq = (np.asarray(x, dtype=dtype) for x in (q, dq, ddq))
    S = q.shape[0]
    rest = rest_kinematics(topo, att, q, dq, ddq, dtype)
    inert = link_inertials(topo, dtype)
    eye4 = np.concatenate([np.zeros((1, 3), dtype=dtype), np.eye(3, dtype=dtype)])
    rep = lambda a: np.tile(a, (4,) + (1,) * (a.ndim - 1))  # noqa: E731
    I3 = np.tile(np.eye(3, dtype=dtype), (4 * S, 1, 1))
    z = np.zeros((4 * S, 3), dtype=dtype)
    N4, k = direct_moment(topo, att, rep(q), rep(dq), rep(ddq), I3, np.repeat(eye4, S, axis=0), z, (0.0, 0.0, 0.0), dtype,
                          rest={key: rep(v) for key, v in rest.items()}, inert=inert)
    N4 = N4.reshape(4, S, 3)
    m, com, Ic = inert
    Io = np.zeros((S, 3, 3), dtype=dtype)
    mc = np.zeros((S, 3), dtype=dtype)
    for l in range(topo.num_links):
        Rl = k["R"][l][:S]
        c = k["p"][l][:S] + _mv(Rl, com[l])
        mc += m[l] * c
        Io += Rl @ Ic[l][None] @ np.swapaxes(Rl, -1, -2) + m[l] * ((c * c).sum(1)[:, None, None] * np.eye(3, dtype=dtype)[None] - c[:, :, None] * c[:, None, :])
    rec = np.zeros((S, REC), dtype=dtype)
    rec[:, OFF_I:OFF_I + 6] = np.stack([Io[:, 0, 0], Io[:, 0, 1], Io[:, 0, 2], Io[:, 1, 1], Io[:, 1, 2], Io[:, 2, 2]], axis=1)
    rec[:, OFF_C0:OFF_C0 + 3] = N4[0]
    B = np.zeros((S, 3, 3), dtype=dtype)
    for i in range(3):
        e = np.zeros(3, dtype=dtype)
        e[i] = 1
        B[:, :, i] = N4[1 + i] - N4[0] - np.cross(e[None], Io[:, :, i])
    rec[:, OFF_B:OFF_B + 9] = B.reshape(S, 9)
    rec[:, OFF_MC:OFF_MC + 3] = mc
    base = int(np.flatnonzero(np.asarray(topo.parent) < 0)[0])
    rec[:, OFF_R:OFF_R + 9] = k["R"][base][:S].reshape(S, 9)
    rec[:, OFF_P:OFF_P + 3] = k["p"][base][:S]
    rec[:, OFF_V:OFF_V + 3] = k["v"][base][:S]
    rec[:, OFF_V + 3:OFF_V + 6] = k["w"][base][:S]
    return rec


def record_moment(rec, R, om, al, gravity):
    """R (c0 + B w + w x (I w) + I dw - mc x (R^T g)) with w = R^T om, dw = R^T al: the direct moment, from the record"""
    dtype = rec.dtype
    Is = rec[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    B = rec[:, OFF_B:OFF_B + 9].reshape(-1, 3, 3)
    w, dw, u = _mtv(R, om), _mtv(R, al), _mtv(R, np.broadcast_to(np.asarray(gravity, dtype=dtype), om.shape))
    Nb = rec[:, OFF_C0:OFF_C0 + 3] + _mv(B, w) + np.cross(w, _mv(Is, w)) + _mv(Is, dw) - np.cross(rec[:, OFF_MC:OFF_MC + 3], u)
    return _mv(R, Nb)


def simulate_from_records(rec, ncand, dt, damping, gravity=(0.0, 0.0, -9.81)):
    """Form (b): the loop on the records alone, O(1) per step and candidate."""
    dtype = rec.dtype.type
    C = int(ncand)
    T = rec.shape[0] // C
    rc = rec.reshape(C, T, REC)
    g = np.asarray(gravity, dtype=dtype)
    z3 = np.zeros((C, 3), dtype=dtype)
    eqlim, swing = dtype(np.deg2rad(EQ_CLIP_DEG)), dtype(np.deg2rad(MAX_SWING_DEG))
    rpy = np.zeros((C, 3), dtype=dtype)
    iters = np.full(C, EQ_MAX_ITER, dtype=np.int64)
    active = np.ones(C, dtype=bool)
    for it in range(EQ_MAX_ITER):
        R = rpy_R(rpy, dtype)
        h = _mv(R, -np.cross(rc[:, 0, OFF_MC:OFF_MC + 3], _mtv(R, np.broadcast_to(g, (C, 3)))))
        done = active & (np.sqrt((h * h).sum(1)) < EQ_TOL)
        iters[done] = it + 1
        active &= ~done
        if not active.any():
            break
        rpy = np.where(active[:, None], np.clip(rpy - dtype(EQ_STEP) * h, -eqlim, eqlim), rpy)
    om = np.zeros((C, 3), dtype=dtype)
    rpy_s, pos_s, vel_s, att_s = (np.zeros((C, T, k), dtype=dtype) for k in (3, 3, 6, 6))
    stats = _new_stats(C)
    for t in range(T):
        r = rc[:, t]
        R = rpy_R(rpy, dtype)
        Is = r[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(C, 3, 3)
        Meff = R @ Is @ np.swapaxes(R, -1, -2) + dtype(damping) * dtype(dt) * np.eye(3, dtype=dtype)[None]
        rhs = -record_moment(r, R, om, z3, g) - dtype(damping) * om
        al = _solve3(Meff, rhs)
        Rwb = R @ r[:, OFF_R:OFF_R + 9].reshape(C, 3, 3)
        pb = _mv(R, r[:, OFF_P:OFF_P + 3])
        rpy_s[:, t] = as_rpy(np.swapaxes(Rwb, -1, -2))
        pos_s[:, t] = pb
        vel_s[:, t, :3] = np.cross(om, pb) + _mv(R, r[:, OFF_V:OFF_V + 3])
        vel_s[:, t, 3:] = om + _mv(R, r[:, OFF_V + 3:OFF_V + 6])
        att_s[:, t, :3], att_s[:, t, 3:] = rpy, om
        if t < T - 1:
            rpy, om = rpy.copy(), om.copy()
            _integrate(rpy, om, al, dtype(dt), swing, stats)
    return _result(rpy_s, pos_s, vel_s, att_s, dtype(dt), iters, stats, C, T)
