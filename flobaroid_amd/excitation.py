"""Batched pieces of the trajectory optimiser's inner loop on top of the fused kernels.

The reference evaluates, per candidate trajectory, ``YBase^T YBase`` -> ``eigvalsh`` (excitation/trajectoryOptimizer.py:248-272)
and, for the analytical gradient, 1 + 3 n regressors per sample in a Python/iDynTree loop spread over worker processes
(excitation/analyticalGradient.py:92-185).  Here both are single device passes:

* ``candidate_dopt``      -- D-optimality of many candidate trajectories from ``Engine.gram_grouped``;
* ``dopt_sensitivities``  -- the worker's ``sens_q, sens_dq, sens_ddq`` from ``Engine.fd_scores``;
* ``candidate_objectives`` -- the whole ``objectiveFunc`` (f, g, soft costs) of many candidates from ``Engine.gram_grouped`` +
  ``Engine.candidate_extrema``; with ``device_spectrum=True`` (``Engine.dopt_terms``) only per-candidate numbers reach the host;
* ``candidate_collision_constraints`` -- its collision block from ``Engine.candidate_capsule_distances`` (``collisionMode: "capsule"``,
  pairs of links with capsules), ``Engine.candidate_box_distances`` (``collisionMode: "box"``, world links, capsule-less links) and
  ``Engine.candidate_hull_distances`` (``collisionMode: "convex"``, the reference's default: convex hulls of the links' meshes; with
  ``Engine.set_hull_meshes`` also ``fullMeshLinks`` and ``collisionMode: "full"``: the triangle meshes themselves, through
  ``Engine.set_large_hull_meshes`` up to 8192 triangles a mesh on hulls of up to 1024 vertices -- KUKA LWR4's ``"full"`` mode);
  ``candidate_objectives(..., collision=...)`` appends it to ``g``;
* ``candidate_dopt_gradient_from_coefficients`` -- the D-optimality term's gradient with respect to the Fourier coefficients of many
  candidates (analyticalGradient.py:538-762) from ``Engine.regressor_weights`` + ``Engine.fd_scores`` + ``Engine.fourier_gradient``;
* ``candidate_collision_gradient`` -- the collision rows of the constraint Jacobian in capsule mode (analyticalGradient.py:955-1027) from
  ``Engine.capsule_distance_gradients`` + ``Engine.fourier_position_chain``; behind keywords the box, hull and triangle-mesh rows
  (``Engine.box_distance_gradients``, ``Engine.hull_distance_gradients``, ``Engine.mesh_distance_gradients``);
* ``candidate_gradients_from_coefficients`` -- everything ``IpoptProblem.gradient`` / ``.jacobian`` need of many candidates: the above plus
  the soft-cost gradients and the position, velocity and torque rows of the constraint Jacobian (analyticalGradient.py:764-953) from
  ``Engine.torque_row_sweep`` + ``Engine.fourier_state_chain``;
* ``candidate_observability`` -- the observability analysis the reference runs on the chosen trajectory (trajectory.py:225-264), per
  candidate from ``Engine.gram_grouped`` + ``Engine.dopt_observability``; ``observability_fields``: its three keys of the trajectory file.
"""
from __future__ import annotations

import numpy as np

from . import estimation as est


def candidate_dopt(engine, states: dict, num_candidates: int, independent_cols, dopt_regularization: float = 1e-4, w=None,
                   YtY_prior=None, device_spectrum: bool = False) -> np.ndarray:
    """Regularised D-optimality -sum(log(max(eig(YBase^T YBase [+ YtY_prior]) + delta, 1e-300))), delta = doptRegularization *
    lambda_max per candidate, of ``num_candidates`` trajectories stacked along the sample axis (equal length each), one fused
    pass (trajectoryOptimizer.py:259-272 per candidate).  ``device_spectrum=True``: the eigenvalues are computed on the device as well
    (``Engine.dopt_terms``) -- the Grams of device states never reach the host; False (default): ``eigvalsh`` on the host, as before."""
    G = engine.gram_grouped(states, int(num_candidates), w=w)
    if device_spectrum:
        return est.d_optimality_batch_terms_device(engine, G, independent_cols, dopt_regularization, YtY_prior)[0]
    G = G.cpu().numpy() if hasattr(G, "cpu") else G
    return est.d_optimality_batch(G, independent_cols, dopt_regularization, YtY_prior)


def dopt_sensitivities(engine, states: dict, W_iner, epsilon: float, W_visc=None, reference_state_carryover: bool = False):
    """``_gradient_worker_chunk`` of analyticalGradient.py:92-185 without its loops: returns ``(sens_q, sens_dq, sens_ddq)``,
    each (S, n), with sens[t, d] = (sum(W_t * Y(state_t + eps e_d)) - sum(W_t * Y(state_t))) / eps.

    ``W_iner`` (S * rows, cols): the D-optimality weight rows of the samples (the reference's ``W_iner`` restricted to the
    identified columns).  ``W_visc`` (S * rows,) optional: the analytic viscous-friction term added to ``sens_dq``
    (analyticalGradient.py:141-143: ``W_visc[t * n_out + fb + d]``).  For a floating base pass the states the reference
    uses there (identity base orientation, zero base twist: rpy = 0, base_vel = 0, base_acc = 0).

    ``reference_state_carryover``: the reference's worker does not reset the kinematic state after its velocity sweep
    (analyticalGradient.py:128-165: ``dq_buf`` is restored but ``setRobotState`` is not called again), so the whole
    acceleration sweep runs with dq_{n-1} + eps still active and every ``sens_ddq[t, d]`` carries the extra term
    ``sens_dq_inertial[t, n-1]`` (exactly: the acceleration part of the regressor does not depend on dq).  False (default)
    returns the clean derivative; True reproduces the reference's numbers (pinned by tests/golden/ref_compute_regressors.npz)."""
    sc = engine.fd_scores(states, W_iner, float(epsilon))
    sc = sc.cpu().numpy() if hasattr(sc, "cpu") else sc
    n = engine.topo.num_dofs
    d = (sc[:, 1:] - sc[:, :1]) / float(epsilon)
    sens_q, sens_dq, sens_ddq = d[:, :n], d[:, n:2 * n].copy(), d[:, 2 * n:3 * n].copy()
    if reference_state_carryover:
        sens_ddq += sens_dq[:, n - 1:n]
    if W_visc is not None:
        fb = engine.rows - n
        Wv = np.asarray(W_visc, dtype=float).reshape(sc.shape[0], engine.rows)
        sens_dq += Wv[:, fb:fb + n]
    return sens_q, sens_dq, sens_ddq


# ------------------------------------------------------------------------------------------------------------------------------------
# Candidate trajectories generated on the device (round 5): the optimiser's search variables are Fourier coefficients; their samples never
# have to exist on the host.
# ------------------------------------------------------------------------------------------------------------------------------------
def fourier_coefficients(a, b, q, nf, wf: float = 1.0, joint_limits=None, use_deg: bool = False):
    """Pack the parameters of ONE candidate as the reference's ``PulsedTrajectory.initWithParams(a, b, q, nf, wf, joint_limits)`` takes
    them (trajectoryGenerator.py:322-383: per-joint coefficient arrays of length nf[i]) into the padded arrays of
    ``Engine.fourier_states``: dict(wf, a (n, nh), b (n, nh), q_offset (n,), q_range (n,) or None).

    classic (``joint_limits`` None, OscillationGenerator 411-460): q_offset = nf * q0;  bounded (BoundedOscillationGenerator 462-510):
    q_offset = q_center = clip(midpoint + q0, lower, upper), q_range = 0.95 * min(q_center - lower, upper - q_center).  ``use_deg``: q
    is given in degrees (the generators convert it)."""
    n = len(nf)
    nh = max(int(k) for k in nf)
    A, B = np.zeros((n, nh)), np.zeros((n, nh))
    for j in range(n):
        A[j, : int(nf[j])] = np.asarray(a[j], dtype=float)[: int(nf[j])]
        B[j, : int(nf[j])] = np.asarray(b[j], dtype=float)[: int(nf[j])]
    q0 = np.deg2rad(np.asarray(q, dtype=float)) if use_deg else np.asarray(q, dtype=float)
    if joint_limits is None:
        return {"wf": float(wf), "a": A, "b": B, "q_offset": np.asarray(nf, dtype=float) * q0, "q_range": None}
    lo = np.array([l[0] for l in joint_limits], dtype=float)
    hi = np.array([l[1] for l in joint_limits], dtype=float)
    qc = np.clip(0.5 * (lo + hi) + q0, lo, hi)
    return {"wf": float(wf), "a": A, "b": B, "q_offset": qc, "q_range": np.minimum(qc - lo, hi - qc) * 0.95}


def _suspended_keys(suspended: dict) -> None:
    unknown = set(suspended) - {"attachment_frame", "att_link", "damping", "x_std"}
    if unknown:
        raise ValueError(f"suspended: unknown keys {sorted(unknown)}")


def suspended_spec(engine, suspended: dict) -> tuple:
    """``(att_link, damping, x_std)`` of a ``suspended=`` argument: a dict with ``x_std`` (the standard parameters whose inertial part
    swings) and optionally ``attachment_frame`` (a link name of the topology; default ``crane_ft``) or ``att_link`` (a link index) and
    ``damping`` (default 2000.0) -- the defaults are what ``simulateTrajectory`` passes (trajectoryGenerator.py:171-187:
    ``floatingBaseAttachmentFrame``, ``suspendedDamping``)."""
    _suspended_keys(suspended)
    if "x_std" not in suspended:
        raise ValueError("suspended: x_std (the standard parameters) is required")
    if "att_link" in suspended and "attachment_frame" in suspended:
        raise ValueError("suspended: give attachment_frame or att_link, not both")
    if "att_link" in suspended:
        att = int(suspended["att_link"])
    else:
        name = suspended.get("attachment_frame", "crane_ft")
        names = list(engine.topo.link_names)
        if name not in names:
            raise ValueError(f"suspended: attachment frame '{name}' is not a link of the topology")
        att = names.index(name)
    x_std = suspended["x_std"]
    return att, float(suspended.get("damping", 2000.0)), getattr(x_std, "xStdModel", x_std)


def candidate_states(engine, candidates: list, T: int, freq: float, device: bool = True, use_deg_vectorised_quirk: bool = False,
                     suspended: dict | None = None, with_info: bool = False) -> dict:
    """States of ``len(candidates)`` candidate trajectories (dicts of ``fourier_coefficients``), T samples each at ``freq`` Hz, as ONE
    stacked batch ready for ``Engine.gram_grouped`` / ``candidate_dopt`` -- what ``computeTrajectoryDynamics`` builds per candidate on the
    host (trajectoryGenerator.py:83-155): joint states from the Fourier series, a stationary base (zero twist / acceleration / rpy).

    ``suspended`` (``suspended_spec``; floating base only): the base swings from a ball joint at the attachment frame instead --
    ``rpy``, ``base_vel``, ``base_acc`` and ``base_position`` come from one ``Engine.suspended_base_motion`` with dt = 1 / freq
    (``simulate_suspended_base_motion`` per candidate, trajectoryGenerator.py:171-187).  None: the stationary base, nothing changed.
    ``with_info`` (with ``suspended`` only): the entry ``suspended_info`` (C, 2) int64 joins the result -- the equilibrium iterations and
    clamp events of ``Engine.suspended_base_motion(..., with_info=True)``; it is no per-sample array: pop it before the states go on.

    ``use_deg_vectorised_quirk``: with ``useDeg`` the reference's vectorised evaluation converts radians with ``deg2rad`` once more
    (lines 126-128 after a block that never produced degrees), i.e. its q, dq, ddq are pi / 180 of the per-sample generators' values;
    True reproduces that output."""
    C = len(candidates)
    n = engine.n
    nh = max(c["a"].shape[1] for c in candidates)
    A, B = np.zeros((C, n, nh)), np.zeros((C, n, nh))
    for i, c in enumerate(candidates):
        A[i, :, : c["a"].shape[1]] = c["a"]
        B[i, :, : c["b"].shape[1]] = c["b"]
    bounded = [c["q_range"] is not None for c in candidates]
    if any(bounded) and not all(bounded):
        raise ValueError("classic and bounded candidates cannot share one batch")
    st = engine.fourier_states([c["wf"] for c in candidates], A, B, np.stack([c["q_offset"] for c in candidates]), int(T), float(freq),
                               q_range=np.stack([c["q_range"] for c in candidates]) if all(bounded) else None, device=device)
    if use_deg_vectorised_quirk:
        st = {k: v * (np.pi / 180.0) for k, v in st.items()}
    if engine.floating:
        S = C * int(T)
        if device:
            import torch

            z = lambda k: torch.zeros((S, k), dtype=torch.float64, device=st["q"].device)  # noqa: E731
        else:
            z = lambda k: np.zeros((S, k))  # noqa: E731
        st.update(base_vel=z(6), base_acc=z(6), rpy=z(3))
    if suspended is not None:
        if not engine.floating:
            raise ValueError("suspended: the engine has no floating base")
        att, damping, x_std = suspended_spec(engine, suspended)
        base = engine.suspended_base_motion(st, C, x_std, att, 1.0 / float(freq), damping, with_info=bool(with_info))
        if with_info:
            base.pop("att_state")
            base["suspended_info"] = base.pop("info")
        st.update(base)
    elif with_info:
        raise ValueError("with_info: the info of the suspended base motion needs suspended=")
    return st


def rest_base_states(states: dict) -> dict:
    """The rest-base view of candidate states: ``q``, ``dq``, ``ddq``, ``sign`` (every other entry too) are the arrays of ``states``
    themselves, ``rpy`` / ``base_rpy``, ``base_vel`` / ``base_velocity`` and ``base_acc`` / ``base_acceleration`` are zeros of their shape in
    their memory space (NumPy or torch) -- the ``fb_identity``, ``fb_zero_twist`` and zero base acceleration the reference's gradient sweeps
    evaluate at (analyticalGradient.py:80-81).  ``base_position`` stays: the sweeps do not read it."""
    out = dict(states)
    for k in ("rpy", "base_rpy", "base_vel", "base_velocity", "base_acc", "base_acceleration"):
        if out.get(k) is not None:
            v = out[k]
            if hasattr(v, "cpu"):
                import torch

                out[k] = torch.zeros_like(v)
            else:
                out[k] = np.zeros_like(np.asarray(v))
    return out


SUSPENDED_BASE_RULES = ("identity", "held")


def _suspended_rule(suspended, suspended_base) -> bool:
    """True when the sweeps run at the rest base (the reference's rule, ``"identity"``, under ``suspended=``)"""
    if suspended_base not in SUSPENDED_BASE_RULES:
        raise ValueError(f"suspended_base: '{suspended_base}' is none of {SUSPENDED_BASE_RULES}")
    if suspended is None and suspended_base != "identity":
        raise ValueError(f"suspended_base='{suspended_base}' without suspended=: the rule applies to the simulated base motion only")
    return suspended is not None and suspended_base == "identity"


def candidate_dopt_from_coefficients(engine, candidates: list, T: int, freq: float, independent_cols, dopt_regularization: float = 1e-4,
                                     YtY_prior=None, friction_sign_threshold: float = 0.02, device_spectrum: bool = False) -> np.ndarray:
    """D-optimality of every candidate without its samples ever leaving the device: Fourier coefficients -> states (``fbr_fourier_states``)
    -> one Gram per candidate (``fbr_gram_grouped``) -> eigenvalues on the host (trajectoryOptimizer.py:240-272 per candidate).
    ``friction_sign_threshold``: the Coulomb column is tanh(dq / threshold) -- callers with an option dict pass
    ``opt.get('frictionSignThreshold', 0.02)`` (helpers.py getFrictionSignSeries, model.py:757), the value ``Model`` uses on the host path.
    ``device_spectrum``: as for ``candidate_dopt``."""
    st = candidate_states(engine, candidates, T, freq, device=True)
    if engine.friction:
        import torch

        st["sign"] = torch.tanh(st["dq"] / float(friction_sign_threshold))
    return candidate_dopt(engine, st, len(candidates), independent_cols, dopt_regularization, YtY_prior=YtY_prior, device_spectrum=device_spectrum)


# ------------------------------------------------------------------------------------------------------------------------------------
# The optimiser's objective per candidate (trajectoryOptimizer.py objectiveFunc, lines 259-475): everything it needs of the samples is the
# per-joint extrema of q, |dq| and |tau| (Engine.candidate_extrema) and, for the collision block in capsule mode, the per-pair minima of the
# capsule distances (Engine.candidate_capsule_distances); the rest is per-candidate host arithmetic.
# ------------------------------------------------------------------------------------------------------------------------------------
def constraint_layout(n: int, min_velocity_constraint: bool, num_collision_pairs: int | None = None) -> dict:
    """Offsets of the blocks of ``g`` (each n long): lower position, upper position, peak velocity, peak torque, [minimum velocity,]
    minimum torque utilisation -- the reference's order; ``len`` = 5 n, or 6 n with the minimum velocity.  With ``num_collision_pairs``
    the collision block (one entry per pair: the smallest distance, positive = free) follows as ``collision`` and ``len`` grows by it."""
    names = ["pos_lower", "pos_upper", "vel", "torque"] + (["min_vel"] if min_velocity_constraint else []) + ["min_torque_util"]
    lay = {k: i * n for i, k in enumerate(names)}
    lay["len"] = len(names) * n
    if num_collision_pairs is not None:
        lay["collision"] = lay["len"]
        lay["len"] += int(num_collision_pairs)
    return lay


def _check_config(config: dict, suspended=None) -> None:
    if config.get("floatingBaseAttachment") == "suspended" and suspended is None:
        raise ValueError("floatingBaseAttachment 'suspended' simulates the base motion with a sequential ODE (suspendedDynamics.py): "
                         "not supported by the batched objective")
    if config.get("identifyGravityParamsOnly"):
        raise ValueError("identifyGravityParamsOnly: the batched objective needs the full torques, which the gravity-only model does not give")


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def objectives_from_extrema(neg_log_det, n_observable, ext: dict, limits: dict, joint_names, config: dict, dopt_scale=None, collision=None,
                            suspended=None) -> dict:
    """``objectiveFunc``'s f, g and soft costs of C candidates from their D-optimality terms and the extrema of ``Engine.candidate_extrema``
    (values and indices, (C, n) each) -- pure host arithmetic.

    ``limits[name]``: ``lower``, ``upper``, ``velocity``, ``torque`` of joint ``name`` (the reference's ``self.limits``); ``joint_names``:
    the n joints in dof order.  ``config`` keys read: ``minVelocityConstraint`` (+ ``minVelocityPercentage``), ``ovrPosLimit`` ({joint:
    [lower_deg, upper_deg]}), ``minTorqueUtilization`` (0.02), ``trajectoryTargetTorqueUtil`` (0.25), ``trajectoryTargetVelocity`` (0).
    ``dopt_scale``: the reference's ``_dopt_scale``; None: 10 / max(|neg_log_det[0]|, 1), what its first call sets.

    Returns, per candidate: ``f`` (C,), ``g`` (C, len) with NaN entries set to 10 (layout: ``constraint_layout``), ``dopt`` (neg_log_det *
    dopt_scale), ``f1`` (torque balance), ``f2`` (position range, already x10 as in the reference), ``f3`` (torque magnitude), ``f4``
    (velocity magnitude), ``n_observable``, ``failed`` (non-finite D-optimality: f starts from 100), ``dopt_scale`` and ``ag_cache`` -- the
    per-candidate entries of the reference's ``_ag_cache`` (``torque_absmax_idx``, ``pos_min_idx``, ``pos_max_idx``, ``vel_absmax_idx``,
    ``vel_absmax``, ``utilization``, ``util_mean``, ``util_std``, ``f1``, ``f3``, ``pos_range_available``).

    ``collision``: the dict ``candidate_collision_constraints`` returns.  Its ``g`` (C, P) is appended after ``min_torque_util`` (layout key
    ``collision``), and ``ag_cache`` gains ``collision_argmin_idx`` (C, P): per pair the main-trajectory sample of its smallest distance
    (-1: none), what the reference's ``_ag_collision_cache`` holds.  None: everything is what it is without the argument.

    ``suspended``: not None says that the extrema come from states with the simulated base motion (``candidate_states(..., suspended=)``);
    ``floatingBaseAttachment: "suspended"`` is then accepted.  The arithmetic is the same."""
    _check_config(config, suspended)
    nld = np.asarray(neg_log_det, dtype=np.float64).reshape(-1)
    C = nld.shape[0]
    e = {k: _host(v) for k, v in ext.items()}
    pos_min, pos_max, vel_absmax, torque_absmax = (e[k].astype(np.float64).reshape(C, -1) for k in ("q_min", "q_max", "dq_absmax", "tau_absmax"))
    n = pos_min.shape[1]
    jn = list(joint_names)
    if len(jn) != n:
        raise ValueError(f"{len(jn)} joint names for {n} joints")
    if dopt_scale is None:
        dopt_scale = 10.0 / max(abs(float(nld[0])), 1.0)
    dopt_scale = float(dopt_scale)

    lower = np.array([limits[j]["lower"] for j in jn], dtype=np.float64)
    upper = np.array([limits[j]["upper"] for j in jn], dtype=np.float64)
    vlim = np.array([limits[j]["velocity"] for j in jn], dtype=np.float64)
    tlim = np.array([limits[j]["torque"] for j in jn], dtype=np.float64)
    lo_c, hi_c = lower.copy(), upper.copy()  # position constraints: ovrPosLimit (degrees) overrides the URDF limits
    ovr = config.get("ovrPosLimit", {})
    for i, j in enumerate(jn):
        pair = ovr.get(j) if isinstance(ovr, dict) else None
        if pair:
            lo_c[i], hi_c[i] = np.deg2rad(pair[0]), np.deg2rad(pair[1])

    minvel = bool(config.get("minVelocityConstraint", False))
    coll_g = None if collision is None else np.asarray(collision["g"], dtype=np.float64).reshape(C, -1)
    lay = constraint_layout(n, minvel, None if coll_g is None else coll_g.shape[1])
    g = np.empty((C, lay["len"]))
    g[:, lay["pos_lower"]:lay["pos_lower"] + n] = lo_c - pos_min
    g[:, lay["pos_upper"]:lay["pos_upper"] + n] = pos_max - hi_c
    g[:, lay["vel"]:lay["vel"] + n] = vel_absmax - vlim
    g[:, lay["torque"]:lay["torque"] + n] = torque_absmax - tlim
    if minvel:
        g[:, lay["min_vel"]:lay["min_vel"] + n] = vlim * config["minVelocityPercentage"] - vel_absmax
    g[:, lay["min_torque_util"]:lay["min_torque_util"] + n] = tlim * config.get("minTorqueUtilization", 0.02) - torque_absmax
    if coll_g is not None:
        g[:, lay["collision"]:] = coll_g
    g[np.isnan(g)] = 10.0

    dopt = nld * dopt_scale
    failed = ~np.isfinite(dopt)
    f = np.where(failed, 100.0, dopt)
    utilization = torque_absmax / tlim
    util_mean = utilization.mean(axis=1)
    util_std = utilization.std(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f1 = np.where(util_mean > 0, util_std / util_mean, 1.0)
    target = config.get("trajectoryTargetTorqueUtil", 0.25)
    f3 = np.maximum(0.0, 1.0 - util_mean / target)
    pos_range_available = upper - lower
    f2 = (1.0 - ((pos_max - pos_min) / pos_range_available).mean(axis=1)) * 10.0
    vel_target = float(config.get("trajectoryTargetVelocity", 0.0))
    f4 = np.maximum(0.0, 1.0 - vel_absmax / vel_target).mean(axis=1) if vel_target > 0 else np.zeros(C)
    f = f + f1 * 10.0 + f3 * 10.0 + f2 + f4 * 10.0
    ag = {"torque_absmax_idx": e["tau_absmax_idx"], "pos_min_idx": e["q_min_idx"], "pos_max_idx": e["q_max_idx"], "vel_absmax_idx": e["dq_absmax_idx"],
          "vel_absmax": vel_absmax, "utilization": utilization, "util_mean": util_mean, "util_std": util_std, "f1": f1, "f3": f3,
          "pos_range_available": pos_range_available}
    if collision is not None:
        ag["collision_argmin_idx"] = np.asarray(collision["argmin"], dtype=np.int64).reshape(C, -1)
    return {"f": f, "g": g, "dopt": dopt, "f1": f1, "f2": f2, "f3": f3, "f4": f4, "n_observable": np.asarray(n_observable).reshape(-1),
            "failed": failed, "dopt_scale": dopt_scale, "ag_cache": ag}


def candidate_collision_constraints(engine, states: dict, ncand: int, config: dict, margins=None, suspended=None, boxes: bool = False,
                                    hulls: bool = False) -> dict:
    """The collision block of ``objectiveFunc`` in capsule mode for ``ncand`` equal candidates stacked in ``states``, for the capsule set of
    the engine (``Engine.set_capsules``; pairs of robot links): per candidate and pair the smallest ``distance - margin`` over

    * every ``collisionCheckStep``-th (3) sample of the main trajectory -- one ``Engine.candidate_capsule_distances`` over ``states``
      (``q``, with a floating base ``rpy`` and optionally ``base_position`` (S, 3)), and
    * with ``transitionDuration`` (3.0) > 0, the minimum-jerk ramps between the zero position and the candidate's first and last sample:
      ``transitionCollisionSamples`` (10) configurations ``s(tau) q`` each, every one at the base poses of six evenly spaced samples and of
      the sample with the largest |rpy| sum -- a second, small device call on states built from the 2 C boundary rows.

    Merged in the reference's order (trajectory first, strict <): a transition configuration wins only when strictly closer.  Returns ``g``
    (C, P) (1e10 where no configuration won), ``idx`` (C, P): the winning sample, or the reference's negative count -1, -2, ... of a
    transition configuration (-1 also stands for "none won": then g is 1e10), ``argmin`` (C, P): the winning main-trajectory sample (-1:
    none), ``dist`` (C, P): the raw main-trajectory minima.  ``margins`` (P,): per-pair clearance subtracted from the distances
    (``_collision_pair_margins``; None: 0).  ``eval_sample``, ``eval_scale``, ``eval_pose`` (C, P) describe the winning configuration
    ``eval_scale * q[eval_sample]`` at the base pose of sample ``eval_pose`` -- (idx, 1, idx) on the main trajectory, (0 or T - 1,
    s(tau), the pose's sample) for a transition configuration, -1 where none won: the arguments of ``Engine.capsule_distance_gradients``
    (``candidate_collision_gradient``).

    ``boxes=True``: the same block for the BOX set of the engine (``Engine.set_boxes``: the pairs the reference sends to its box
    fallback -- ``collisionMode: "box"``, world links, capsule-less links) from ``Engine.candidate_box_distances``; the main trajectory and
    the transition configurations are walked once per set, each with its set's distance call.  ``hulls=True``: the same for the HULL set
    (``Engine.set_hulls``: every pair of ``collisionMode: "convex"``) from ``Engine.candidate_hull_distances``; with triangle meshes
    attached to that set (``Engine.set_hull_meshes``: ``fullMeshLinks``, ``collisionMode: "full"``) the pairs of a meshed link come back as
    mesh distances, 0.0 where they touch and never negative.

    ``suspended``: not None says that ``states`` carry the simulated base motion of the suspended base (``rpy`` and ``base_position`` of
    ``candidate_states(..., suspended=)``); ``floatingBaseAttachment: "suspended"`` is then accepted.  The poses of the main trajectory
    and the seven base poses of the transition configurations are those of ``states``, as in the reference."""
    _check_config(config, suspended)
    if boxes and hulls:
        raise ValueError("boxes=True and hulls=True: one set per call")
    distances = engine.candidate_hull_distances if hulls else (engine.candidate_box_distances if boxes else engine.candidate_capsule_distances)
    return _collision_constraints(engine, distances, states, ncand, config, margins)


def _collision_constraints(engine, distances, states, ncand, config, margins):
    """``candidate_collision_constraints`` with the distance call of one set: ``distances(states, ncand, step, base_pos=)``"""
    C = int(ncand)
    q = states["q"]
    S, n = int(q.shape[0]), int(q.shape[1])
    T = S // max(C, 1)
    rpy = states.get("rpy", states.get("base_rpy")) if engine.floating else None
    bpos = states.get("base_position") if engine.floating else None
    main = distances(states, C, int(config.get("collisionCheckStep", 3)), base_pos=bpos)
    dist, idx = _host(main["dist"]), _host(main["idx"]).astype(np.int64)
    P = dist.shape[1]
    m = np.zeros(P) if margins is None else np.asarray(margins, dtype=np.float64).reshape(P)
    g = np.where(idx >= 0, dist - m, 1e10)
    out_idx = idx.copy()
    ev_sample, ev_scale, ev_pose = idx.copy(), np.where(idx >= 0, 1.0, -1.0), idx.copy()
    ns = int(config.get("transitionCollisionSamples", 10))
    if config.get("transitionDuration", 3.0) > 0 and ns > 0 and S == C * T and T > 0:
        torch_in = hasattr(q, "cpu")
        if torch_in:
            import torch

            dev = lambda a, dt=None: torch.as_tensor(a, dtype=dt, device=q.device)  # noqa: E731
            expand = lambda a, shape: a.expand(*shape).reshape(-1, shape[-1]).contiguous()  # noqa: E731
        else:
            dev = lambda a, dt=None: np.asarray(a)  # noqa: E731
            expand = lambda a, shape: np.ascontiguousarray(np.broadcast_to(a, shape).reshape(-1, shape[-1]))  # noqa: E731
        # base poses of the transition configurations: six evenly spaced samples and the extreme swing, in sample order.  The reference
        # drops repeated samples; here all seven are evaluated (equal candidates) and a repeated pose, whose distances are the same,
        # never wins against its first occurrence: `rank` is a pose's position among the distinct ones.
        lin = np.linspace(0, T - 1, 6).astype(int)
        if rpy is not None:
            r3 = rpy.reshape(C, T, 3)
            ext = _host(abs(r3).sum(-1).argmax(1)).astype(int)
            poses = np.sort(np.concatenate([np.tile(lin, (C, 1)), ext[:, None]], axis=1), axis=1)
        else:
            poses = np.sort(np.concatenate([lin, [0]]))[None].repeat(C, axis=0)
        rank = np.cumsum(np.concatenate([np.zeros((C, 1), dtype=int), (poses[:, 1:] != poses[:, :-1]).astype(int)], axis=1), axis=1)
        nuniq = rank[:, -1] + 1
        npose = poses.shape[1] if rpy is not None else 1  # (fixed base: every pose gives the same distances, one is evaluated)
        tau = (np.arange(ns) + 1) / (ns + 1)
        sv = 10.0 * tau**3 - 15.0 * tau**4 + 6.0 * tau**5
        qb = q.reshape(C, T, n)[:, [0, T - 1]]  # (C, 2, n)
        qt = qb[:, :, None, None, :] * dev(sv, qb.dtype if torch_in else None)[None, None, :, None, None]
        shape = (C, 2, ns, npose)
        st_tr = {"q": expand(qt, shape + (n,))}
        bp_tr = None
        if rpy is not None:
            ci, pi = dev(np.arange(C)[:, None]), dev(poses)
            st_tr["rpy"] = expand(r3[ci, pi][:, None, None], shape + (3,))
            if bpos is not None:
                bp_tr = expand(bpos.reshape(C, T, 3)[ci, pi][:, None, None], shape + (3,))
        tr = distances(st_tr, C, 1, base_pos=bp_tr)
        dt, it = _host(tr["dist"]), _host(tr["idx"]).astype(np.int64)
        kk = np.maximum(it, 0)
        ref_idx = -((kk // npose) * nuniq[:, None] + np.take_along_axis(rank, kk % npose, axis=1) + 1)
        gt = dt - m
        take = (it >= 0) & (gt < g)
        g = np.where(take, gt, g)
        out_idx = np.where(take, ref_idx, out_idx)
        # the winning transition configuration s(tau) q[boundary] at the base pose of sample poses[.]: flat index ((boundary, tau), pose)
        tr_sample = np.where(kk // (ns * npose) == 0, 0, T - 1)
        ev_sample = np.where(take, tr_sample, ev_sample)
        ev_scale = np.where(take, sv[(kk // npose) % ns], ev_scale)
        ev_pose = np.where(take, np.take_along_axis(poses, kk % npose, axis=1) if rpy is not None else tr_sample, ev_pose)
    return {"g": g, "idx": out_idx, "argmin": idx, "dist": dist, "eval_sample": ev_sample.astype(np.int64), "eval_scale": ev_scale,
            "eval_pose": ev_pose.astype(np.int64)}


def _has_box_pairs(collision) -> bool:
    return collision is not None and len(collision.get("box_pairs", ())) > 0


def _has_hull_pairs(collision) -> bool:
    return collision is not None and len(collision.get("hull_pairs", ())) > 0


def _has_meshes(collision) -> bool:
    return collision is not None and bool(collision.get("meshes"))


def _refuse_large_mesh_gradient(collision) -> None:
    """without ``large_mesh_gradient=True`` a set built with ``collision_set(..., large_meshes=True)`` is refused by every gradient entry
    point, whatever its other ``*_gradient`` keywords say, by the names and triangle counts of its meshes above ``FBR_MAX_MESH_TRIANGLES``
    triangles or on hulls above ``FBR_MAX_HULL_VERTICES`` vertices (the message is the one from before that gradient was built: callers
    match it)"""
    from .collision import FBR_MAX_HULL_VERTICES, FBR_MAX_MESH_TRIANGLES

    if not (_has_meshes(collision) and collision.get("large_meshes")):
        return
    why = []
    for h, t in collision["meshes"].items():
        hull = collision["hulls"][int(h)]
        nt, nv = len(np.asarray(t).reshape(-1, 9)), len(hull.vertices)
        if nt > FBR_MAX_MESH_TRIANGLES or nv > FBR_MAX_HULL_VERTICES:
            why.append(f"{hull.link_name} ({nt} triangles on a hull of {nv} vertices)")
    raise ValueError("gradients on the device do not cover triangle meshes of more than 256 triangles or on hulls of more than 128 vertices: "
                     "the collision set was built with large_meshes=True and has " + (", ".join(why) if why else "no such mesh")
                     + "; the constraint values are served (Engine.set_large_hull_meshes), their gradients are not built")


def _wants_large_mesh_gradient(config, collision, large_mesh_gradient) -> bool:
    """True when ``large_mesh_gradient=True`` selects the rows of ``Engine.large_mesh_distance_gradients``: a set built with
    ``large_meshes``, hull pairs only, and a configuration that uses the meshes (``collisionMode: "full"``, or ``fullMeshLinks`` in
    ``"convex"``).  False without the keyword: every refusal of before then holds.  The keyword with anything else raises and says which
    condition fails."""
    if not large_mesh_gradient:
        return False
    mode = config.get("collisionMode", "capsule")
    if mode in ("capsule", "box"):
        raise ValueError(f"large_mesh_gradient=True: collisionMode '{mode}' has no triangle meshes (they belong to collisionMode 'full' and to "
                         "fullMeshLinks in collisionMode 'convex')")
    if not (_has_meshes(collision) and collision.get("large_meshes")):
        serves = ("mesh_gradient=True serves a set with triangle meshes attached without it" if _has_meshes(collision) else
                  "large_hull_gradient=True serves a set of hulls above 128 vertices without meshes" if _large_hulls(collision) else
                  "hull_gradient=True serves a set of hulls only")
        raise ValueError("large_mesh_gradient=True: the collision set was not built with large_meshes=True "
                         "(flobaroid_amd.collision.collision_set(..., hulls=, meshes=, large_meshes=True)); " + serves)
    if mode != "full" and not config.get("fullMeshLinks"):
        raise ValueError(f"large_mesh_gradient=True: collisionMode '{mode}' without fullMeshLinks does not use the meshes of the collision set")
    if "hulls" not in collision or not _has_hull_pairs(collision) or "columns" not in collision:
        raise ValueError("large_mesh_gradient=True: the collision set needs hull pairs "
                         "(flobaroid_amd.collision.collision_set(..., hulls=, meshes=, large_meshes=True))")
    if (np.asarray(collision["columns"], dtype=np.int64).reshape(-1, 2)[:, 0] != 2).any():
        raise ValueError("large_mesh_gradient=True: the collision set has capsule or box pairs")
    return True


def _refuse_mesh_gradient(collision) -> None:
    """without ``mesh_gradient=True`` a set with triangle meshes is refused by the names of its meshed links (the message is the one from
    before the mesh gradient was built: callers match it)"""
    if _has_meshes(collision):
        links = [collision["hulls"][int(h)].link_name for h in collision["meshes"]]
        raise ValueError(f"gradients on the device do not cover triangle meshes: the collision set has meshes on {links} (fullMeshLinks / "
                         "collisionMode 'full'); the constraint values are served, their gradients are not built")


def _wants_mesh_gradient(config, collision, mesh_gradient) -> bool:
    """True when ``mesh_gradient=True`` selects the rows of ``Engine.mesh_distance_gradients``: a set with triangle meshes and a
    configuration that uses them (``collisionMode: "full"``, or ``fullMeshLinks`` in ``"convex"``).  False without the keyword: every
    refusal of before then holds.  The keyword with anything else raises."""
    if not mesh_gradient:
        return False
    mode = config.get("collisionMode", "capsule")
    if mode in ("capsule", "box"):
        raise ValueError(f"mesh_gradient=True: collisionMode '{mode}' has no triangle meshes (they belong to collisionMode 'full' and to "
                         "fullMeshLinks in collisionMode 'convex')")
    if not _has_meshes(collision):
        raise ValueError("mesh_gradient=True: the collision set has no triangle meshes (flobaroid_amd.collision.collision_set(..., hulls=, "
                         "meshes=)); hull_gradient=True serves a set of hulls only")
    if mode != "full" and not config.get("fullMeshLinks"):
        raise ValueError(f"mesh_gradient=True: collisionMode '{mode}' without fullMeshLinks does not use the meshes of the collision set")
    if "hulls" not in collision or not _has_hull_pairs(collision) or "columns" not in collision:
        raise ValueError("mesh_gradient=True: the collision set needs hull pairs (flobaroid_amd.collision.collision_set(..., hulls=, meshes=))")
    if (np.asarray(collision["columns"], dtype=np.int64).reshape(-1, 2)[:, 0] != 2).any():
        raise ValueError("mesh_gradient=True: the collision set has capsule or box pairs")
    return True


_NO_HULL_GRADIENT = ("gradients on the device cover capsule and box pairs only: the collision set has hull pairs (collisionMode 'convex'; the "
                     "reference differentiates those by central differences, which is not built for hulls)")


def _wants_hull_gradient(config, collision, hull_gradient) -> bool:
    """True when ``hull_gradient=True`` selects the hull rows: ``collisionMode: "convex"`` and a set of hull pairs only.  Every other
    combination goes on to the refusals that hold without the keyword."""
    _refuse_mesh_gradient(collision)
    if not hull_gradient or config.get("collisionMode", "capsule") != "convex":
        return False
    if collision is None or "hulls" not in collision or not _has_hull_pairs(collision) or "columns" not in collision:
        raise ValueError("hull_gradient=True: collisionMode 'convex' needs a collision set with hull pairs "
                         "(flobaroid_amd.collision.collision_set(..., hulls=))")
    if (np.asarray(collision["columns"], dtype=np.int64).reshape(-1, 2)[:, 0] != 2).any():
        raise ValueError("hull_gradient=True: the collision set of collisionMode 'convex' has capsule or box pairs")
    return True


def _large_hulls(collision) -> list:
    """[(link or world name, vertices)] of the hulls of the set above ``FBR_MAX_HULL_VERTICES`` vertices, which ``Engine.set_hulls`` takes
    with ``large=True`` only"""
    from .collision import FBR_MAX_HULL_VERTICES

    if collision is None or "hulls" not in collision:
        return []
    out = []
    for h in collision["hulls"]:
        if not hasattr(h, "vertices") and not (isinstance(h, (tuple, list)) and len(h) >= 4):
            continue  # (not a hull as Engine.set_hulls takes it: that call says so)
        v = h.vertices if hasattr(h, "vertices") else h[3]
        if len(v) > FBR_MAX_HULL_VERTICES:
            out.append(((h.link_name or h.name) if hasattr(h, "vertices") else h[0], len(v)))
    return out


def _refuse_large_hull_gradient(collision) -> None:
    """hulls above ``FBR_MAX_HULL_VERTICES`` vertices are served for distances only: every gradient entry point refuses the set by the
    names and counts of those hulls, whatever its ``*_gradient`` keywords say"""
    big = _large_hulls(collision)
    if big and _has_hull_pairs(collision):
        raise ValueError("gradients on the device do not cover hulls of more than 128 vertices: the collision set has "
                         + ", ".join(f"{name} ({nv} vertices)" for name, nv in big)
                         + "; the constraint values are served (Engine.set_hulls(..., large=True)), their gradients are not built")


def _wants_large_hull_gradient(config, collision, large_hull_gradient) -> bool:
    """True when ``large_hull_gradient=True`` selects the rows of ``Engine.large_hull_distance_gradients``: ``collisionMode: "convex"``, a set
    of hull pairs only, at least one hull above ``FBR_MAX_HULL_VERTICES`` vertices and no triangle meshes.  False without the keyword:
    every refusal of before then holds.  The keyword with anything else raises and says which condition fails."""
    if not large_hull_gradient:
        return False
    mode = config.get("collisionMode", "capsule")
    if mode != "convex":
        raise ValueError(f"large_hull_gradient=True: collisionMode '{mode}' is not 'convex', the only mode whose pairs are hulls of more than 128 "
                         "vertices")
    if _has_meshes(collision) or config.get("fullMeshLinks"):
        raise ValueError("large_hull_gradient=True: the collision set has triangle meshes or the configuration names fullMeshLinks (meshes on large "
                         "hulls are not built; mesh_gradient=True serves a set of small hulls with meshes)")
    if collision is None or "hulls" not in collision or not _has_hull_pairs(collision) or "columns" not in collision:
        raise ValueError("large_hull_gradient=True: collisionMode 'convex' needs a collision set with hull pairs "
                         "(flobaroid_amd.collision.collision_set(..., hulls=))")
    if (np.asarray(collision["columns"], dtype=np.int64).reshape(-1, 2)[:, 0] != 2).any():
        raise ValueError("large_hull_gradient=True: the collision set has capsule or box pairs")
    if not _large_hulls(collision):
        raise ValueError("large_hull_gradient=True: the collision set has no hull above 128 vertices; hull_gradient=True serves such a set")
    return True


def _collision_block(engine, states, ncand, config, collision, suspended=None):
    """``collision``: dict with ``capsules``, ``pairs`` and optionally ``margins``, and for sets with boxes ``boxes``, ``box_pairs``, ``columns``
    and optionally ``center_in_link_axes``, for sets with hulls ``hulls``, ``hull_pairs``, ``columns`` and ``offset_in_link_axes``
    (``flobaroid_amd.collision.collision_set``).  Every set with pairs is installed and walked with its own distance call, and the
    (C, P_set) results are merged into the reference's pair order."""
    if collision is None:
        return None
    mode = config.get("collisionMode", "capsule")
    if mode == "full" or config.get("fullMeshLinks"):
        # triangle meshes ride on the hull set: the pairs, their order and the margins are those of convex mode
        if not _has_meshes(collision):
            raise ValueError(f"collisionMode 'full' and fullMeshLinks {list(config.get('fullMeshLinks', []))} need a collision set with triangle "
                             "meshes (flobaroid_amd.collision.collision_set(..., hulls=, meshes=))")
        if mode == "full":
            mode = "convex"
    if mode not in ("capsule", "box", "convex"):
        raise ValueError("collision constraints on the device cover collisionMode 'capsule', 'box', 'convex' and 'full' only")
    if mode == "convex" and "hulls" not in collision:
        raise ValueError("collisionMode 'convex' needs a collision set with hulls (flobaroid_amd.collision.collision_set(..., hulls=))")
    if mode != "convex" and _has_hull_pairs(collision):
        raise ValueError(f"collisionMode '{mode}': the collision set was built for convex mode (it has hull pairs)")
    if "columns" not in collision:
        if mode != "capsule":
            raise ValueError("collisionMode 'box' needs a collision set with boxes (flobaroid_amd.collision.collision_set(..., boxes=))")
        engine.set_capsules(collision["capsules"], collision["pairs"])
        return candidate_collision_constraints(engine, states, ncand, config, margins=collision.get("margins"), suspended=suspended)
    cols = np.asarray(collision["columns"], dtype=np.int64).reshape(-1, 2)
    P = cols.shape[0]
    if mode == "box" and (cols[:, 0] == 0).any():
        raise ValueError("collisionMode 'box': the collision set was built for capsule mode (it has capsule pairs)")
    m = np.zeros(P) if collision.get("margins") is None else np.asarray(collision["margins"], dtype=np.float64).reshape(P)
    out = None
    if mode == "convex" and (cols[:, 0] != 2).any():
        raise ValueError("collisionMode 'convex': the collision set has capsule or box pairs")
    for which in (0, 1, 2):
        sel = np.nonzero(cols[:, 0] == which)[0]
        if sel.size == 0:
            continue
        if which == 0:
            engine.set_capsules(collision["capsules"], collision["pairs"])
        elif which == 1:
            engine.set_boxes(collision["boxes"], collision["box_pairs"], center_in_link_axes=bool(collision.get("center_in_link_axes", False)))
        else:
            kw = {"meshes": collision["meshes"]} if _has_meshes(collision) else {}
            if _large_hulls(collision):  # (the keyword only then: engines of before know nothing of it)
                kw["large"] = True
            if kw.get("meshes") and collision.get("large_meshes"):  # (Engine.set_large_hull_meshes: the same rule)
                kw["large_meshes"] = True
            engine.set_hulls(collision["hulls"], collision["hull_pairs"], offset_in_link_axes=bool(collision.get("offset_in_link_axes", False)), **kw)
        part = candidate_collision_constraints(engine, states, ncand, config, margins=m[sel], suspended=suspended, boxes=which == 1, hulls=which == 2)
        if out is None:
            out = {k: np.zeros((np.asarray(v).shape[0], P), dtype=np.asarray(v).dtype) for k, v in part.items()}
        for k, v in part.items():
            out[k][:, sel] = np.asarray(v)[:, cols[sel, 1]]
    if out is None:
        raise ValueError("the collision set has no pairs")
    return out


def candidate_objectives(engine, states: dict, ncand: int, independent_cols, x_std, limits: dict, joint_names, config: dict, dopt_scale=None,
                         YtY_prior=None, vel_sign=None, collision=None, suspended=None, device_spectrum: bool = False) -> dict:
    """``objectives_from_extrema`` of ``ncand`` equal candidates stacked in ``states``: one ``gram_grouped`` (D-optimality, lambda_max,
    n_observable per candidate with ``doptRegularization``, default 1e-4) and one ``candidate_extrema`` (the a-priori torques of ``x_std``
    reduced on the device) over the same states.  ``vel_sign``: Stribeck friction, as for ``Engine.inverse_dynamics``.  ``collision``
    (``flobaroid_amd.collision.collision_set``: capsules, pairs, margins): the collision block of capsule mode is appended to ``g``
    (``candidate_collision_constraints``); None: no collision block, every array as without the argument.  ``suspended``: not None says
    that ``states`` carry the simulated base motion (``candidate_states(..., suspended=)``: ``rpy``, ``base_vel``, ``base_acc``, and
    ``base_position`` for the collision block); ``floatingBaseAttachment: "suspended"`` is then accepted.  ``device_spectrum=True``: the
    D-optimality terms come from one ``Engine.dopt_terms`` call on the grouped Gram where ``gram_grouped`` left it -- with device states
    only per-candidate numbers reach the host; False (default): the Gram is brought to the host for ``eigvalsh``, every array as before.
    The keyword with ``useBasisProjection`` in ``config`` raises: the host route serves that case."""
    return _candidate_objective_parts(engine, states, ncand, independent_cols, x_std, limits, joint_names, config, dopt_scale, YtY_prior, vel_sign,
                                      collision, suspended, device_spectrum)[0]


def _candidate_objective_parts(engine, states, ncand, independent_cols, x_std, limits, joint_names, config, dopt_scale, YtY_prior, vel_sign, collision,
                               suspended=None, device_spectrum=False, with_weights=False):
    """``candidate_objectives`` together with what the gradients reuse: (result, the grouped Gram on the host -- under ``device_spectrum``
    where ``gram_grouped`` left it, a tensor for device states --, the collision block or None, the weight matrices or None).
    ``with_weights`` (under ``device_spectrum``): the one ``Engine.dopt_terms`` call also forms -2 (M + delta I)^-1, in the memory space of
    the Gram, for the caller to scale by ``dopt_scale``, which is known only after the terms."""
    _check_config(config, suspended)
    Cm = None
    if device_spectrum:
        _refuse_basis_projection(config)
        G = engine.gram_grouped(states, int(ncand))
        t = engine.dopt_terms(G, independent_cols, config.get("doptRegularization", 1e-4), prior=YtY_prior, weights=bool(with_weights))
        nld, nobs, Cm = _host(t["neg_log_det"]), _host(t["n_observable"]), t.get("Cmat")
    else:
        G = _host(engine.gram_grouped(states, int(ncand)))
        nld, _, nobs = est.d_optimality_batch_terms(G, independent_cols, config.get("doptRegularization", 1e-4), YtY_prior)
    ext = engine.candidate_extrema(states, int(ncand), x_std, vel_sign=vel_sign)
    coll = _collision_block(engine, states, ncand, config, collision, suspended)
    return objectives_from_extrema(nld, nobs, ext, limits, joint_names, config, dopt_scale, collision=coll, suspended=suspended), G, coll, Cm


def candidate_objectives_from_coefficients(engine, candidates: list, T: int, freq: float, model_or_x_std, independent_cols, limits: dict,
                                           joint_names, config: dict, dopt_scale=None, YtY_prior=None, collision=None, suspended=None,
                                           device_spectrum: bool = False) -> dict:
    """``candidate_objectives`` from Fourier coefficients (``fourier_coefficients`` dicts): states generated on the device
    (``candidate_states``), the Coulomb column tanh(dq / ``frictionSignThreshold``) as ``candidate_dopt_from_coefficients`` sets it and
    ``vel_sign`` = dq under Stribeck friction -- only per-candidate arrays come back to the host.  ``model_or_x_std``: the a-priori standard
    parameters, or an object with ``xStdModel`` (``Model``).  ``suspended`` (``suspended_spec``): the base motion of every candidate is
    simulated on the device (``candidate_states(..., suspended=)``) and ``floatingBaseAttachment: "suspended"`` accepted; None: the
    stationary base, and that configuration is refused.  ``device_spectrum``: as for ``candidate_objectives`` -- True keeps the Grams in
    HBM, so that only per-candidate numbers reach the host."""
    _check_config(config, suspended)
    x_std = getattr(model_or_x_std, "xStdModel", model_or_x_std)
    st = _coefficient_states(engine, candidates, T, freq, config.get("frictionSignThreshold", 0.02), suspended)
    vel_sign = st["dq"] if getattr(engine, "stribeck", 0.0) > 0 else None
    return candidate_objectives(engine, st, len(candidates), independent_cols, x_std, limits, joint_names, config, dopt_scale=dopt_scale,
                                YtY_prior=YtY_prior, vel_sign=vel_sign, collision=collision, suspended=suspended, device_spectrum=device_spectrum)


# ------------------------------------------------------------------------------------------------------------------------------------
# The D-optimality term of the optimiser's gradient per candidate (analyticalGradient.py compute_analytical_gradient, Phases 1, A and B,
# lines 538-762): weight rows on the device (Engine.regressor_weights), the finite-difference sweep (Engine.fd_scores) and the chain with
# the Jacobian of the Fourier series (Engine.fourier_gradient).  The collision rows of the constraint Jacobian: candidate_collision_gradient
# below; Phase C and the whole gradient: candidate_gradients_from_coefficients at the end.  The suspended base (``suspended=``): the weights
# come from the swung states; the sweeps run at the rest base (``suspended_base="identity"``, the reference's rule: rest_base_states) or at the
# swung states held fixed (``"held"``).  Neither differentiates the base motion itself, as the reference does not.
# ------------------------------------------------------------------------------------------------------------------------------------
def _refuse_basis_projection(config, what: str = "device_spectrum=True", host: str = "device_spectrum=False, dopt_weight_matrices(..., B=B)") -> None:
    """``device_spectrum=True`` covers YBase = Y[:, independent_cols] only: a configuration that switches ``useBasisProjection`` on (a
    truthy value; ``Model`` itself sets the key to 0) is refused.  ``what`` / ``host``: the route that refuses and the one that serves."""
    if config.get("useBasisProjection"):
        raise ValueError(f"{what} does not cover useBasisProjection (a basis-projection matrix B: YBase = Y B): the host route "
                         f"({host}) serves that case")


def dopt_weight_matrices(G, independent_cols, dopt_regularization: float = 1e-4, dopt_scale=1.0, YtY_prior=None, B=None):
    """The constant matrices of ``Engine.regressor_weights`` for C candidates from their Grams ``G`` (C, Pa, Pa) (``Engine.gram_grouped``):
    returns ``(Cmat, cols)``, ``Cmat`` (C, ncols, ncols), such that ``W_c = Y_c[:, cols] @ Cmat[c]`` are the reference's weight rows
    ``W_std = R_dopt Pb^T`` (analyticalGradient.py:538-565) restricted to ``cols``:

        Cmat[c] = -2 scale Pb (Pb^T G_c Pb [+ YtY_prior] + delta_c I)^-1 Pb^T,      delta_c = dopt_regularization * lambda_max,

    lambda_max the largest eigenvalue of ``Pb^T G_c Pb [+ YtY_prior]`` (floored at 1e-30) -- the delta of ``estimation.d_optimality_batch``.
    Without ``B`` the base regressor is ``Y[:, independent_cols]`` (Pb selects columns): ``cols = independent_cols`` and Cmat[c] is the
    regularised inverse itself.  With ``B`` (P, nb) (``useBasisProjection``: YBase = Y B) ``cols`` is every column and
    ``Cmat[c] = -2 scale B (B^T G_c B [+ prior] + delta_c I)^-1 B^T``.  ``dopt_scale``: a number or one per candidate.

    delta is HELD FIXED in the derivative, as the reference does: the weights are the gradient of -scale logdet(M + delta_0 I) at
    delta_0 = delta(theta_0), not of the objective with delta following lambda_max(theta)."""
    G = np.asarray(G, dtype=np.float64)
    if G.ndim == 2:
        G = G[None]
    nC = G.shape[0]
    scale = np.broadcast_to(np.asarray(dopt_scale, dtype=np.float64), (nC,))
    if B is None:
        cols = np.asarray(independent_cols, dtype=np.int64)
        M = G[:, cols[:, None], cols[None, :]]
    else:
        B = np.asarray(B, dtype=np.float64)
        P = B.shape[0]
        cols = np.arange(P, dtype=np.int64)
        M = B.T[None] @ G[:, :P, :P] @ B[None]
    if YtY_prior is not None:
        M = M + np.asarray(YtY_prior, dtype=np.float64)[None]
    ev = np.linalg.eigvalsh(M)
    delta = float(dopt_regularization) * np.maximum(ev[:, -1], 1e-30)
    Minv = np.linalg.inv(M + delta[:, None, None] * np.eye(M.shape[1])[None])
    Cm = Minv if B is None else B[None] @ Minv @ B.T[None]
    return np.ascontiguousarray(-2.0 * scale[:, None, None] * Cm), cols.astype(np.int32)


def candidate_dopt_gradient_from_coefficients(engine, candidates: list, T: int, freq: float, independent_cols, dopt_regularization: float = 1e-4,
                                              dopt_scale=None, YtY_prior=None, epsilon: float = 1e-7, subsample: int = 1,
                                              friction_sign_threshold: float = 0.02, max_weight_bytes: int = 2**31, suspended=None,
                                              suspended_base: str = "identity", device_spectrum: bool = False):
    """D-optimality term and its gradient for every candidate (``fourier_coefficients`` dicts) without a sample leaving the device:
    coefficients -> states (``fbr_fourier_states``) -> one Gram per candidate (``fbr_gram_grouped``) -> ``dopt_weight_matrices`` on the host
    -> for chunks of whole candidates whose weight rows fit ``max_weight_bytes``: ``regressor_weights`` -> ``fd_scores`` -> forward
    differences on the device -> ``fourier_gradient``.  Only per-candidate numbers and the matrices C cross PCIe.

    Returns ``(f, grad)``: ``f`` (C,) = ``dopt_scale`` * the value of ``candidate_dopt_from_coefficients`` (``dopt_scale`` None: 1) and a
    dict of arrays ``wf`` (C,), ``q_offset`` (C, n), ``q_range`` (C, n) (zeros for classic candidates), ``a`` / ``b`` (C, n, nh), the
    derivatives of f with respect to the entries of the ``fourier_coefficients`` dicts, delta held fixed (``dopt_weight_matrices``);
    columns that only pad ``a`` / ``b`` to a common width are removed (nh = the widest candidate's).

    ``subsample`` = k sweeps the samples 0, k, 2 k, ... only and scales the result by k (``analyticalGradientSubsample``); the Gram, f and
    C always use every sample.  Friction engines: the viscous column is linear in dq and sits in W, so the sweep carries its derivative
    (the reference adds it analytically, ``W_visc``); the Coulomb sign tanh(dq / threshold) is held at its baseline value, as there.

    ``suspended`` (``suspended_spec``; floating base only): the base motion of every candidate is simulated on the device
    (``candidate_states(..., suspended=)``); the Gram, f, C and the weight rows take those swung states.  ``suspended_base``: where the
    sweep runs -- ``"identity"`` (default, the reference's rule, analyticalGradient.py:80-81, 107-111): the same q, dq, ddq and sign with
    rpy, base_vel and base_acc zero (``rest_base_states``); ``"held"``: the swung states, i.e. the partial derivative with the simulated
    base trajectory frozen.  Neither differentiates the base motion.  Any other value, or ``"held"`` without ``suspended=``, raises.

    ``device_spectrum=True``: f and the matrices C come from one ``Engine.dopt_terms(..., weights=True)`` on the Grams in HBM and C goes to
    ``regressor_weights`` as a tensor -- only per-candidate numbers cross PCIe; False (default): the host route above, every array as
    before."""
    rest = _suspended_rule(suspended, suspended_base)
    st = _coefficient_states(engine, candidates, T, freq, friction_sign_threshold, suspended)
    scale = 1.0 if dopt_scale is None else float(dopt_scale)
    if device_spectrum:
        G = engine.gram_grouped(st, len(candidates))
        terms = engine.dopt_terms(G, independent_cols, dopt_regularization, prior=YtY_prior, scale=scale, weights=True)
        Cm = terms["Cmat"]
        return _host(terms["neg_log_det"]) * scale, _dopt_gradient(engine, st, G, candidates, T, freq, independent_cols, dopt_regularization, scale,
                                                                  YtY_prior, epsilon, subsample, max_weight_bytes, rest_base=rest, weights=Cm)
    G = _host(engine.gram_grouped(st, len(candidates)))
    nld = est.d_optimality_batch(G, independent_cols, dopt_regularization, YtY_prior)
    return nld * scale, _dopt_gradient(engine, st, G, candidates, T, freq, independent_cols, dopt_regularization, scale, YtY_prior, epsilon, subsample,
                                       max_weight_bytes, rest_base=rest)


def _coefficient_states(engine, candidates, T, freq, friction_sign_threshold, suspended=None, with_info=False):
    """``candidate_states`` on the device with the Coulomb column tanh(dq / threshold) of a friction engine"""
    st = candidate_states(engine, candidates, int(T), freq, device=True, suspended=suspended, with_info=with_info)
    if engine.friction:
        import torch

        st["sign"] = torch.tanh(st["dq"] / float(friction_sign_threshold))
    return st


def _gradient_dict(g, n: int, nh: int) -> dict:
    """the columns [wf | q_offset (n) | q_range (n) | a (n, nh) | b (n, nh)] of ``g`` (..., 1 + 2 n + 2 n nh) as the dict of the gradients"""
    lead = g.shape[:-1]
    return {"wf": g[..., 0].copy(), "q_offset": g[..., 1:1 + n].copy(), "q_range": g[..., 1 + n:1 + 2 * n].copy(),
            "a": g[..., 1 + 2 * n:1 + 2 * n + n * nh].reshape(lead + (n, nh)).copy(), "b": g[..., 1 + 2 * n + n * nh:].reshape(lead + (n, nh)).copy()}


def _dopt_gradient(engine, st, G, candidates, T, freq, independent_cols, dopt_regularization, scale, YtY_prior, epsilon, subsample, max_weight_bytes,
                   rest_base=False, weights=None):
    """the gradient dict of ``candidate_dopt_gradient_from_coefficients`` from the candidates' device states and grouped Gram;
    ``rest_base``: the weights from ``st``, the scores from its rest-base view; ``weights``: the matrices C when the caller has them
    (``Engine.dopt_terms``: ``G`` is then not read), else ``dopt_weight_matrices`` forms them on the host"""
    import torch

    C = len(candidates)
    n = engine.n
    T, k = int(T), max(int(subsample), 1)
    if weights is not None:
        Cm, cols = weights, np.asarray(independent_cols, dtype=np.int32)
    else:
        Cm, cols = dopt_weight_matrices(G, independent_cols, dopt_regularization, scale, YtY_prior)
    Ts = (T + k - 1) // k
    if k > 1:
        st = {key: v.reshape(C, T, -1)[:, ::k].reshape(C * Ts, -1).contiguous() for key, v in st.items()}
    at = rest_base_states(st) if rest_base else st
    per_cand = Ts * engine.rows * engine.cols * 8
    cc = max(1, min(C, int(max_weight_bytes) // max(per_cand, 1)))
    sens = torch.empty((3, C * Ts, n), dtype=torch.float64, device=st["q"].device)
    W = torch.empty((cc * Ts * engine.rows, engine.cols), dtype=torch.float64, device=st["q"].device)
    for c0 in range(0, C, cc):
        c1 = min(C, c0 + cc)
        sub = {key: v[c0 * Ts:c1 * Ts] for key, v in st.items()}
        Wc = W[: (c1 - c0) * Ts * engine.rows]
        engine.regressor_weights(sub, c1 - c0, Cm[c0:c1], cols=cols, out=Wc)
        sc = engine.fd_scores({key: v[c0 * Ts:c1 * Ts] for key, v in at.items()} if rest_base else sub, Wc, float(epsilon))
        d = (sc[:, 1:] - sc[:, :1]) * (k / float(epsilon))
        sens[:, c0 * Ts:c1 * Ts] = d.reshape(-1, 3, n).permute(1, 0, 2)
    nh = max(c["a"].shape[1] for c in candidates)
    A, B = np.zeros((C, n, nh)), np.zeros((C, n, nh))
    for i, c in enumerate(candidates):
        A[i, :, : c["a"].shape[1]] = c["a"]
        B[i, :, : c["b"].shape[1]] = c["b"]
    bounded = all(c["q_range"] is not None for c in candidates)
    g = _host(engine.fourier_gradient([c["wf"] for c in candidates], A, B, sens[0], sens[1], sens[2], Ts, float(freq),
                                      q_range=np.stack([c["q_range"] for c in candidates]) if bounded else None, tstride=k))
    return _gradient_dict(g, n, nh)


def gradient_to_optimizer_variables(grad: dict, candidate: dict, nf, use_deg: bool = False, bounded: bool | None = None, exact: bool = False,
                                    joint_limits=None, q0=None) -> np.ndarray:
    """One candidate's gradient (the entries ``wf`` (), ``q_offset`` (n,), ``q_range`` (n,), ``a`` / ``b`` (n, nh) of
    ``candidate_dopt_gradient_from_coefficients``, i.e. ``{k: v[c] for k, v in grad.items()}``) on the reference's variable vector
    ``[wf | q0 (n) | a_0[:nf_0] .. a_{n-1}[:nf_{n-1}] | b_0[:nf_0] ..]`` (trajectoryOptimizer.py; analyticalGradient.py:675-762), with the
    reference's own conventions for q0: classic ``q_offset = nf * q0`` enters as ``nf_d * deg_factor`` (deg_factor = pi / 180 with
    ``use_deg``); bounded through ``q_center`` only, ``deg_factor``.

    ``exact`` (bounded): adds what the reference leaves out -- ``q_center = clip(mid + q0, lo, hi)`` has derivative 0 where it clips and
    ``q_range = 0.95 min(q_center - lo, hi - q_center)`` moves with q0 by +-0.95.  Needs ``joint_limits`` [(lo, hi)] and ``q0`` (the
    variable's value, in degrees with ``use_deg``)."""
    nf = [int(x) for x in nf]
    n = len(nf)
    if bounded is None:  # the candidate's own form
        bounded = candidate.get("q_range") is not None
    deg = np.pi / 180.0 if use_deg else 1.0
    gq = np.asarray(grad["q_offset"], dtype=np.float64).reshape(n)
    if not bounded:
        dq0 = gq * np.asarray(nf, dtype=np.float64) * deg
    else:
        dq0 = gq * deg
        if exact:
            lo = np.array([l[0] for l in joint_limits], dtype=np.float64)
            hi = np.array([l[1] for l in joint_limits], dtype=np.float64)
            raw = 0.5 * (lo + hi) + np.asarray(q0, dtype=np.float64) * deg
            inside = ((raw > lo) & (raw < hi)).astype(np.float64)
            qc = np.clip(raw, lo, hi)
            dqr = 0.95 * np.where(qc - lo <= hi - qc, 1.0, -1.0)
            dq0 = (gq + np.asarray(grad["q_range"], dtype=np.float64).reshape(n) * dqr) * inside * deg
    ga, gb = np.asarray(grad["a"], dtype=np.float64), np.asarray(grad["b"], dtype=np.float64)
    return np.concatenate([[float(np.asarray(grad["wf"]))], dq0] + [ga[j, :nf[j]] for j in range(n)] + [gb[j, :nf[j]] for j in range(n)])


# ------------------------------------------------------------------------------------------------------------------------------------
# The collision rows of the constraint Jacobian per candidate (analyticalGradient.py:955-1027, capsule.py capsule_distance_and_gradient):
# the distance gradient at each pair's winning configuration (Engine.capsule_distance_gradients) chained with the position Jacobian of the
# Fourier series at that configuration's time (Engine.fourier_position_chain).  Two deliberate deviations from the reference:
# the lever arm of a closest point is v + omega x r, and a transition configuration s(tau) q[boundary] is chained with s(tau) times the
# Jacobian at the boundary sample, not with the Jacobian at an index wrapped round from the end of the time array.
# ------------------------------------------------------------------------------------------------------------------------------------
def _padded_coefficients(candidates: list, n: int):
    C = len(candidates)
    nh = max(c["a"].shape[1] for c in candidates)
    A, B = np.zeros((C, n, nh)), np.zeros((C, n, nh))
    for i, c in enumerate(candidates):
        A[i, :, : c["a"].shape[1]] = c["a"]
        B[i, :, : c["b"].shape[1]] = c["b"]
    bounded = [c["q_range"] is not None for c in candidates]
    if any(bounded) and not all(bounded):
        raise ValueError("classic and bounded candidates cannot share one batch")
    return A, B, nh, (np.stack([c["q_range"] for c in candidates]) if all(bounded) else None)


def _chain_positions(engine, candidates, freq, sample, scale, grad_q, max_bytes):
    """rows ``grad_q`` (C, P, n) at ``scale * q[sample]`` chained with the position Jacobian of the series, over chunks of whole candidates:
    (C, P, 1 + 2 n + 2 n nh) on the host, and nh"""
    n = engine.n
    A, B, nh, qr = _padded_coefficients(candidates, n)
    wf = np.array([c["wf"] for c in candidates], dtype=np.float64)
    C, P = int(sample.shape[0]), int(sample.shape[1])
    E = 1 + 2 * n + 2 * n * nh
    cc = max(1, min(C, int(max_bytes) // max(P * E * 8, 1)))
    out = np.empty((C, P, E))
    for c0 in range(0, C, cc):
        c1 = min(C, c0 + cc)
        out[c0:c1] = _host(engine.fourier_position_chain(wf[c0:c1], A[c0:c1], B[c0:c1], sample[c0:c1], grad_q[c0:c1], float(freq),
                                                         scale=scale[c0:c1], q_range=None if qr is None else qr[c0:c1]))
    return out, nh


def candidate_collision_gradient(engine, states: dict, ncand: int, candidates: list, freq: float, config: dict, collision: dict,
                                 constraints: dict | None = None, max_bytes: int = 2**31, box_gradient: bool = False, epsilon=None,
                                 hull_gradient: bool = False, mesh_gradient: bool = False, large_hull_gradient: bool = False,
                                 large_mesh_gradient: bool = False, suspended=None) -> dict:
    """The collision block ``g = distance - margin`` (C, P) of ``ncand`` equal candidates stacked in ``states`` and its derivative with
    respect to the entries of the candidates' ``fourier_coefficients`` dicts, from which ``states`` were generated at ``freq`` Hz
    (``candidate_states``).  ``collision``: capsules, pairs and optionally margins (``flobaroid_amd.collision.collision_set``);
    ``constraints``: the result of ``candidate_collision_constraints`` for the same states and set, when the caller has it (None: computed).

    Returns ``{"g": (C, P), "grad": {"wf": (C, P), "q_offset": (C, P, n), "q_range": (C, P, n) (zeros for classic candidates), "a" / "b":
    (C, P, n, nh)}, "grad_q": (C, P, n)}`` as NumPy arrays: the margins are constants, so a row of ``grad`` is the derivative of the
    pair's distance at its winning configuration, held fixed (the reference's rule); a pair without a winner has a zero row.  ``grad_q`` is
    the derivative with respect to the evaluated configuration itself.  The chain runs over chunks of whole candidates whose output stays
    within ``max_bytes``; columns that only pad ``a`` / ``b`` to a common width are removed (nh = the widest candidate's).  The base pose
    of a floating base is held constant, as in the reference.

    ``box_gradient=False``: a set with box pairs (``collision_set(..., boxes=, world_boxes=)``) raises ``ValueError``, as does any
    ``collisionMode`` but ``"capsule"``.  ``box_gradient=True``: ``collisionMode`` ``"capsule"`` or ``"box"``; the rows of the box pairs
    (world links, capsule-less links, every pair of box mode) are the reference's central differences of the box distance over
    ``epsilon`` (None: ``config.get("analyticalGradientEpsilon", 1e-7)``) from ``Engine.box_distance_gradients``.  Each of the two sets of
    ``collision["columns"]`` is installed, evaluated at its columns of the constraint block (``constraints``: then the merged block of
    ``candidate_objectives``) and chained; ``g``, ``grad`` and ``grad_q`` come back in the reference's pair order.  A set without
    ``columns`` goes the capsule way unchanged.  Joints off a pair's path are exact zeros where the reference has difference noise.

    ``hull_gradient=False``: ``collisionMode: "convex"`` and every set with hull pairs raise ``ValueError``.  ``hull_gradient=True`` with
    ``collisionMode: "convex"`` (the reference's default): the set must have hull pairs and only those; the hull set is installed and the
    rows are the reference's central differences of the hull distance over ``epsilon`` (as above) from ``Engine.hull_distance_gradients``
    at the evaluation points of the constraint block, transitions included, in the reference's pair order.  In the modes ``"capsule"`` and
    ``"box"`` the keyword changes nothing: a set with hull pairs stays refused there.  A set with triangle meshes (``fullMeshLinks``,
    ``collisionMode: "full"``) is refused by the names of its meshed links, whatever the keywords above.

    ``mesh_gradient=True`` serves such a set: it needs triangle meshes in ``collision`` and a configuration that uses them
    (``collisionMode: "full"``, or ``fullMeshLinks`` in ``"convex"``), installs the hull set with its meshes and takes the rows from
    ``Engine.mesh_distance_gradients`` exactly as ``hull_gradient=True`` takes them from the hull call: the reference's central
    differences of the mesh distance, the plain pairs of the set as the hull call returns them.  A pair in intersection has distance 0.0
    and an exactly zero row (a mesh carries no penetration depth).  The keyword with a set without meshes, or in the modes ``"capsule"``
    and ``"box"``, raises ``ValueError``.

    ``large_hull_gradient=False``: a set with a hull above 128 vertices (KUKA LWR4's hulls of visual meshes) is refused by the names and
    vertex counts of those hulls, whatever the keywords above.  ``True`` serves it: ``collisionMode: "convex"``, a set of hull pairs only
    with at least one such hull and no triangle meshes; the hull set is installed with ``large=True`` and the rows of ALL its pairs come
    from ``Engine.large_hull_distance_gradients`` exactly as ``hull_gradient=True`` takes them from the hull call (``hull_gradient`` may
    then be either value).  The keyword with anything else raises ``ValueError`` and says which condition fails.

    ``large_mesh_gradient=False``: a set built with ``collision_set(..., large_meshes=True)`` (KUKA LWR4 in ``collisionMode: "full"``) is
    refused by the names and triangle counts of its meshes, whatever the keywords above.  ``True`` serves it: a set with ``large_meshes``,
    hull pairs only, ``collisionMode: "full"`` or ``fullMeshLinks`` in ``"convex"``; the hull set is installed with ``large_meshes=True``
    (and ``large=True`` where a hull exceeds 128 vertices) and the rows of ALL its pairs come from
    ``Engine.large_mesh_distance_gradients`` (the other three keywords may then be either value): the mesh pairs through the trees, the
    plain pairs as the hull and the large-hull call return them.  The keyword with anything else raises ``ValueError``, says which
    condition fails and, where one exists, names the keyword that serves the set.

    ``suspended``: not None says that ``states`` carry the simulated base motion (``candidate_states(..., suspended=)``: ``rpy`` and
    ``base_position``); ``floatingBaseAttachment: "suspended"`` is then accepted, under every keyword above.  Every row is taken at the
    base pose of sample ``eval_pose`` of the constraint block, held constant: the pose the winning evaluation was made at, for a
    transition winner one of the seven representative poses.  That deviates from the reference on purpose: it differentiates a transition
    winner at the pose of sample 0 (analyticalGradient.py:960-971), a different point from the one whose distance is the constraint
    value.  The coupling through the base dynamics is neglected, as there."""
    _check_config(config, suspended)
    tree_rows = _wants_large_mesh_gradient(config, collision, large_mesh_gradient)
    if not tree_rows:
        _refuse_large_mesh_gradient(collision)
    large_rows = not tree_rows and _wants_large_hull_gradient(config, collision, large_hull_gradient)
    if not (large_rows or tree_rows):
        _refuse_large_hull_gradient(collision)
    mesh_rows = not (large_rows or tree_rows) and _wants_mesh_gradient(config, collision, mesh_gradient)
    if not (mesh_rows or tree_rows):
        _refuse_mesh_gradient(collision)
    mode = config.get("collisionMode", "capsule")
    if tree_rows or large_rows or mesh_rows or _wants_hull_gradient(config, collision, hull_gradient):
        C, n = int(ncand), engine.n
        bpos = states.get("base_position") if engine.floating else None
        cons = constraints if constraints is not None else _collision_block(engine, states, C, config, collision, suspended)
        eps = float(config.get("analyticalGradientEpsilon", 1e-7) if epsilon is None else epsilon)
        cols = np.asarray(collision["columns"], dtype=np.int64).reshape(-1, 2)
        sel = np.argsort(cols[:, 1], kind="stable")  # (the set's own pair order)
        smp, sc, pose = (np.ascontiguousarray(np.asarray(cons[k])[:, sel]) for k in ("eval_sample", "eval_scale", "eval_pose"))
        kw = {"meshes": collision["meshes"]} if mesh_rows else ({"large": True} if large_rows else {})
        if tree_rows:
            kw = dict({"large": True} if _large_hulls(collision) else {}, meshes=collision["meshes"], large_meshes=True)
        engine.set_hulls(collision["hulls"], collision["hull_pairs"], offset_in_link_axes=bool(collision.get("offset_in_link_axes", False)), **kw)
        gradients = (engine.large_mesh_distance_gradients if tree_rows else engine.large_hull_distance_gradients if large_rows else
                     engine.mesh_distance_gradients if mesh_rows else engine.hull_distance_gradients)
        dg = gradients(states, C, smp, scale=sc, pose_sample=pose, base_pos=bpos, epsilon=eps)
        part, nh = _chain_positions(engine, candidates, freq, smp, sc, dg["grad_q"], max_bytes)
        out, grad_q = np.zeros((C, cols.shape[0], part.shape[2])), np.zeros((C, cols.shape[0], n))
        out[:, sel] = part
        grad_q[:, sel] = _host(dg["grad_q"])
        return {"g": np.asarray(cons["g"]), "grad": _gradient_dict(out, n, nh), "grad_q": grad_q}
    if _has_hull_pairs(collision) and mode in ("capsule", "box"):
        raise ValueError(_NO_HULL_GRADIENT)
    if not box_gradient:
        if mode != "capsule":
            raise ValueError("the collision gradient on the device covers collisionMode 'capsule' only (no mesh code: DESIGN 9)")
        if _has_box_pairs(collision):
            raise ValueError("the collision gradient on the device covers capsule pairs only: the set has box pairs (the reference differentiates "
                             "those by central differences; box_gradient=True does the same on the device)")
    elif mode not in ("capsule", "box"):
        raise ValueError("the collision gradient on the device covers collisionMode 'capsule' and 'box' only (no mesh code: DESIGN 9)")
    C, n = int(ncand), engine.n
    bpos = states.get("base_position") if engine.floating else None
    if not box_gradient or "columns" not in collision:
        if mode != "capsule":
            raise ValueError("collisionMode 'box' needs a collision set with boxes (flobaroid_amd.collision.collision_set(..., boxes=))")
        engine.set_capsules(collision["capsules"], collision["pairs"])
        cons = constraints if constraints is not None else candidate_collision_constraints(engine, states, C, config, margins=collision.get("margins"),
                                                                                           suspended=suspended)
        dg = engine.capsule_distance_gradients(states, C, cons["eval_sample"], scale=cons["eval_scale"], pose_sample=cons["eval_pose"], base_pos=bpos)
        out, nh = _chain_positions(engine, candidates, freq, cons["eval_sample"], cons["eval_scale"], dg["grad_q"], max_bytes)
        return {"g": np.asarray(cons["g"]), "grad": _gradient_dict(out, n, nh), "grad_q": np.asarray(_host(dg["grad_q"]))}
    cons = constraints if constraints is not None else _collision_block(engine, states, C, config, collision, suspended)
    eps = float(config.get("analyticalGradientEpsilon", 1e-7) if epsilon is None else epsilon)
    cols = np.asarray(collision["columns"], dtype=np.int64).reshape(-1, 2)
    P = cols.shape[0]
    out, grad_q, nh = None, np.zeros((C, P, n)), 0
    for which in (0, 1):
        sel = np.nonzero(cols[:, 0] == which)[0]
        if sel.size == 0:
            continue
        sel = sel[np.argsort(cols[sel, 1], kind="stable")]  # (the set's own pair order)
        smp, sc, pose = (np.ascontiguousarray(np.asarray(cons[k])[:, sel]) for k in ("eval_sample", "eval_scale", "eval_pose"))
        if which == 0:
            engine.set_capsules(collision["capsules"], collision["pairs"])
            dg = engine.capsule_distance_gradients(states, C, smp, scale=sc, pose_sample=pose, base_pos=bpos)
        else:
            engine.set_boxes(collision["boxes"], collision["box_pairs"], center_in_link_axes=bool(collision.get("center_in_link_axes", False)))
            dg = engine.box_distance_gradients(states, C, smp, scale=sc, pose_sample=pose, base_pos=bpos, epsilon=eps)
        part, nh = _chain_positions(engine, candidates, freq, smp, sc, dg["grad_q"], max_bytes)
        if out is None:
            out = np.zeros((C, P, part.shape[2]))
        out[:, sel] = part
        grad_q[:, sel] = _host(dg["grad_q"])
    if out is None:
        raise ValueError("the collision set has no pairs")
    return {"g": np.asarray(cons["g"]), "grad": _gradient_dict(out, n, nh), "grad_q": grad_q}


def candidate_collision_gradient_from_coefficients(engine, candidates: list, T: int, freq: float, config: dict, collision: dict,
                                                   max_bytes: int = 2**31, box_gradient: bool = False, hull_gradient: bool = False,
                                                   mesh_gradient: bool = False, large_hull_gradient: bool = False,
                                                   large_mesh_gradient: bool = False, suspended=None) -> dict:
    """``candidate_collision_gradient`` from Fourier coefficients (``fourier_coefficients`` dicts): the states are generated on the device
    (``candidate_states``) and never leave it; only the per-pair rows come back.  ``box_gradient``, ``hull_gradient``, ``mesh_gradient``,
    ``large_hull_gradient``, ``large_mesh_gradient``: as there.  ``suspended`` (``suspended_spec``): the states carry the simulated base
    motion (``candidate_states(..., suspended=)``) and every row is taken at the pose its winning evaluation was made at, as there."""
    _check_config(config, suspended)
    st = candidate_states(engine, candidates, int(T), float(freq), device=True, suspended=suspended)
    return candidate_collision_gradient(engine, st, len(candidates), candidates, freq, config, collision, max_bytes=max_bytes,
                                        box_gradient=box_gradient, hull_gradient=hull_gradient, mesh_gradient=mesh_gradient,
                                        large_hull_gradient=large_hull_gradient, large_mesh_gradient=large_mesh_gradient, suspended=suspended)


def constraint_gradient_to_optimizer_variables(grad: dict, candidate: dict, nf, use_deg: bool = False, bounded: bool | None = None, exact: bool = False,
                                               joint_limits=None, q0=None) -> np.ndarray:
    """``gradient_to_optimizer_variables`` for every row of ONE candidate's constraint block at once: ``grad`` holds ``wf`` (P,),
    ``q_offset`` / ``q_range`` (P, n), ``a`` / ``b`` (P, n, nh) (``{k: v[c] for k, v in candidate_collision_gradient(...)["grad"].items()}``);
    returns (P, n_vars) on the reference's variable vector ``[wf | q0 (n) | a_0[:nf_0] .. | b_0[:nf_0] ..]`` -- the block that goes at rows
    ``constraint_layout(...)["collision"]`` of its ``con_grad``.  The other arguments as for ``gradient_to_optimizer_variables``."""
    nf = [int(x) for x in nf]
    n = len(nf)
    if bounded is None:
        bounded = candidate.get("q_range") is not None
    deg = np.pi / 180.0 if use_deg else 1.0
    gq = np.asarray(grad["q_offset"], dtype=np.float64).reshape(-1, n)
    if not bounded:
        dq0 = gq * np.asarray(nf, dtype=np.float64)[None] * deg
    else:
        dq0 = gq * deg
        if exact:
            lo = np.array([l[0] for l in joint_limits], dtype=np.float64)
            hi = np.array([l[1] for l in joint_limits], dtype=np.float64)
            raw = 0.5 * (lo + hi) + np.asarray(q0, dtype=np.float64) * deg
            inside = ((raw > lo) & (raw < hi)).astype(np.float64)
            qc = np.clip(raw, lo, hi)
            dqr = 0.95 * np.where(qc - lo <= hi - qc, 1.0, -1.0)
            dq0 = (gq + np.asarray(grad["q_range"], dtype=np.float64).reshape(-1, n) * dqr[None]) * inside[None] * deg
    ga, gb = np.asarray(grad["a"], dtype=np.float64), np.asarray(grad["b"], dtype=np.float64)
    return np.concatenate([np.asarray(grad["wf"], dtype=np.float64).reshape(-1, 1), dq0] + [ga[:, j, :nf[j]] for j in range(n)]
                          + [gb[:, j, :nf[j]] for j in range(n)], axis=1)


# ------------------------------------------------------------------------------------------------------------------------------------
# Phase C of the analytical gradient (analyticalGradient.py:764-953) per candidate: the soft costs f1 .. f4 and the position, velocity, torque,
# minimum-velocity and minimum-torque-utilisation rows of the constraint Jacobian.  Every one of them is a combination of 4 n rows per
# candidate, each the derivative of ONE extremum with respect to the joint states at the sample where it is reached, chained with the
# Jacobian of the Fourier series at that sample's time (Engine.fourier_state_chain); the torque rows come from forward differences of
# Engine.torque_row_sweep.  Deliberate deviations from the reference: the wf column is analytic (there: central differences
# of the whole trajectory); the torque Jacobians are the clean derivative (the reference's acceleration sweep still carries dq_{n-1} + eps
# from its velocity sweep, see dopt_sensitivities: no flag reproduces that here); candidates whose D-optimality term failed get the
# soft-cost gradient only.
# ------------------------------------------------------------------------------------------------------------------------------------
def candidate_torque_jacobians(engine, states: dict, ncand: int, sample, x_std, epsilon: float = 1e-7, vel_sign=None, rest_base: bool = False) -> dict:
    """The ``torque_sens`` of the reference's gradient worker (``_dopt_gradient_worker_func``, the ``need_torque`` branches, analyticalGradient.py:114-183) for ``ncand`` equal candidates stacked in ``states``:
    joint n's torque at sample ``sample[c, n]`` of candidate c and its forward differences over the joint states, from one
    ``Engine.torque_row_sweep``.  Returns ``tau`` (C, n), the baseline values whose ``np.sign`` is the reference's ``sign_n``, and
    ``dtau_dq``, ``dtau_ddq_state``, ``dtau_dddq`` (C, n, n): row n holds the derivatives of tau_n with respect to q, dq and ddq (the
    reference's names), in the memory space of the states.  The Coulomb sign series, ``vel_sign`` and the base state are held at the
    sample's values; the clean derivative, without the reference's carried-over dq_{n-1} + eps in the acceleration sweep.

    ``rest_base=True`` (the suspended base under the reference's rule, analyticalGradient.py:107-125): the three derivative arrays come from
    the sweep at ``rest_base_states(states)`` -- rpy, base_vel, base_acc zero, everything else the sample's own.  ``tau`` stays the torque at
    the states passed in (the swung ones, whose sign is ``sign_n``): one ``Engine.inverse_dynamics`` over the C n gathered samples."""
    n = engine.n
    sw = engine.torque_row_sweep(rest_base_states(states) if rest_base else states, int(ncand), sample, x_std, float(epsilon), vel_sign=vel_sign)
    d = (sw[..., 1:] - sw[..., :1]) / float(epsilon)
    tau = sw[..., 0]
    if rest_base:
        C, q = int(ncand), states["q"]
        keys = [k for k in ("q", "dq", "ddq", "rpy", "base_rpy", "base_vel", "base_velocity", "base_acc", "base_acceleration", "sign")
                if states.get(k) is not None]
        flat = (_like(q, sample, np.int64).reshape(C, n) + _like(q, np.arange(C) * (int(q.shape[0]) // max(C, 1)), np.int64)[:, None]).reshape(-1)
        take = lambda a: a[flat].contiguous() if hasattr(a, "cpu") else np.ascontiguousarray(np.asarray(a)[flat])  # noqa: E731
        tau = engine.inverse_dynamics({k: take(states[k]) for k in keys}, x_std, vel_sign=None if vel_sign is None else take(vel_sign))
        fb = engine.rows - n
        tau = _like(sw, tau).reshape(C, n, engine.rows)[:, list(range(n)), list(range(fb, fb + n))]  # (row n of the sample gathered for joint n)
    return {"tau": tau, "dtau_dq": d[..., :n], "dtau_ddq_state": d[..., n:2 * n], "dtau_dddq": d[..., 2 * n:]}


def _like(ref, a, dtype=None):
    """``a`` as an array of ``ref``'s kind: a torch tensor on ``ref``'s device, or NumPy; float64 unless ``dtype`` (a NumPy type) says int64"""
    if hasattr(ref, "cpu"):
        import torch

        return torch.as_tensor(a, dtype=torch.int64 if dtype == np.int64 else torch.float64, device=ref.device)
    return np.asarray(_host(a), dtype=dtype or np.float64)


def _cat(parts, axis: int):
    if hasattr(parts[0], "cpu"):
        import torch

        return torch.cat(parts, dim=axis)
    return np.concatenate(parts, axis=axis)


def constraint_chain_rows(ag_cache: dict, torque_jacobians: dict, vel_at_peak):
    """The 4 n rows per candidate that Phase C chains with the Jacobian of the Fourier series, in the order [|tau| peak (n) | position
    minimum (n) | position maximum (n) | |dq| peak (n)]: returns ``(sample, grad_q, grad_dq, grad_ddq)`` -- (C, 4 n) int64 and three
    (C, 4 n, n) arrays, the arguments of ``Engine.fourier_state_chain`` -- of the kind (NumPy / torch) of ``torque_jacobians``.

    torque rows: sign(tau_n) (dtau_dq[n], dtau_ddq_state[n], dtau_dddq[n]) at ``torque_absmax_idx[n]``; position rows: e_n on q at
    ``pos_min_idx[n]`` / ``pos_max_idx[n]``; velocity rows: sign(dq_n) e_n on dq at ``vel_absmax_idx[n]``, ``vel_at_peak`` (C, n) being the
    velocities there."""
    tau = torque_jacobians["tau"]
    C, n = int(tau.shape[0]), int(tau.shape[1])
    sgn = lambda v: (v > 0) * _like(tau, 1.0) - (v < 0) * _like(tau, 1.0)  # noqa: E731  (np.sign for both kinds; a NaN gives 0)
    st = sgn(tau)[:, :, None]
    eye = _like(tau, np.eye(n))[None] + 0.0 * st
    zero = 0.0 * eye
    sv = sgn(_like(tau, vel_at_peak))[:, :, None]
    sample = _cat([_like(tau, ag_cache[k], np.int64).reshape(C, n) for k in ("torque_absmax_idx", "pos_min_idx", "pos_max_idx", "vel_absmax_idx")], 1)
    grad_q = _cat([st * torque_jacobians["dtau_dq"], eye, eye, zero], 1)
    grad_dq = _cat([st * torque_jacobians["dtau_ddq_state"], zero, zero, sv * eye], 1)
    grad_ddq = _cat([st * torque_jacobians["dtau_dddq"], zero, zero, zero], 1)
    return sample, grad_q, grad_dq, grad_ddq


def constraint_gradients_from_rows(ag_cache: dict, torque_jacobians: dict, vel_at_peak, chain, limits: dict, joint_names, config: dict,
                                   suspended=None) -> dict:
    """The arithmetic of Phase C (analyticalGradient.py:764-953) for C candidates, arrays in and arrays out (NumPy or torch, the kind of
    ``torque_jacobians``), no engine.  ``ag_cache``: the entry ``ag_cache`` of ``objectives_from_extrema``; ``torque_jacobians``:
    ``candidate_torque_jacobians`` at ``ag_cache["torque_absmax_idx"]``; ``vel_at_peak`` (C, n): dq_n at ``vel_absmax_idx[n]``; ``limits``,
    ``joint_names``, ``config`` as for ``objectives_from_extrema``.  ``chain(sample, grad_q, grad_dq, grad_ddq)`` chains the rows of
    ``constraint_chain_rows`` with the Jacobian of the trajectory series and returns (C, 4 n, E) -- ``Engine.fourier_state_chain`` with the
    candidates' coefficients bound, or any restatement of it; E is whatever parameter axis it produces.

    Returns ``obj_grad`` (C, E) = 10 df1 + 10 df3 + df2 + 10 df4 (f2 carries its factor 10 already) with the reference's conditions -- f1
    only where util_mean > 0 and util_std > 0, f3 only where f3 > 0, f4 only with ``trajectoryTargetVelocity`` > 0 and for joints with
    vel_absmax < the target -- its terms ``df1`` .. ``df4`` (C, E) before those factors (``df2`` of the x10 f2), and ``con_grad``
    (C, 5 n or 6 n, E) in ``constraint_layout`` order: -dq at the argmin, +dq at the argmax, sign d(dq), d|tau|, [-sign d(dq) with
    ``minVelocityConstraint``,] -d|tau|.

    ``suspended``: not None says that ``ag_cache`` and ``torque_jacobians["tau"]`` come from states with the simulated base motion
    (``candidate_torque_jacobians(..., rest_base=)`` chooses where the derivatives are taken); ``floatingBaseAttachment: "suspended"`` is
    then accepted.  The arithmetic is the same."""
    _check_config(config, suspended)
    if suspended is not None:
        _suspended_keys(suspended)
    tau = torque_jacobians["tau"]
    n = int(tau.shape[1])
    jn = list(joint_names)
    if len(jn) != n:
        raise ValueError(f"{len(jn)} joint names for {n} joints")
    rows = chain(*constraint_chain_rows(ag_cache, torque_jacobians, vel_at_peak))
    dT, dPmin, dPmax, dV = rows[:, :n], rows[:, n:2 * n], rows[:, 2 * n:3 * n], rows[:, 3 * n:]
    A = lambda k: _like(rows, ag_cache[k])  # noqa: E731
    tlim = _like(rows, np.array([limits[j]["torque"] for j in jn], dtype=np.float64))
    util, mean, std, f1, f3 = A("utilization"), A("util_mean"), A("util_std"), A("f1"), A("f3")
    one = _like(rows, 1.0)
    dutil = dT / tlim[None, :, None]
    on1 = ((mean > 0) & (std > 0)) * one
    m1, s1 = mean * on1 + (1.0 - on1), std * on1 + (1.0 - on1)  # (1 where the term is off: nothing is divided by zero)
    df1_dutil = ((util - mean[:, None]) / s1[:, None] - f1[:, None]) / (n * m1[:, None])
    df1 = on1[:, None] * (df1_dutil[:, :, None] * dutil).sum(1)
    df3 = ((f3 > 0) * one)[:, None] * (-1.0 / config.get("trajectoryTargetTorqueUtil", 0.25)) * dutil.mean(1)
    df2 = -10.0 * ((dPmax - dPmin) / A("pos_range_available")[None, :, None]).mean(1)
    vt = float(config.get("trajectoryTargetVelocity", 0.0))
    df4 = 0.0 * df2
    if vt > 0:
        df4 = (-1.0 / (n * vt)) * (((A("vel_absmax") < vt) * one)[:, :, None] * dV).sum(1)
    blocks = [-dPmin, dPmax, dV, dT] + ([-dV] if config.get("minVelocityConstraint", False) else []) + [-dT]
    return {"obj_grad": 10.0 * df1 + 10.0 * df3 + df2 + 10.0 * df4, "df1": df1, "df2": df2, "df3": df3, "df4": df4, "con_grad": _cat(blocks, 1)}


def candidate_gradients_from_coefficients(engine, candidates: list, T: int, freq: float, model_or_x_std, independent_cols, limits: dict, joint_names,
                                          config: dict, dopt_scale=None, YtY_prior=None, collision=None, epsilon=None, subsample: int = 1,
                                          box_gradient: bool = False, hull_gradient: bool = False, mesh_gradient: bool = False,
                                          large_hull_gradient: bool = False, large_mesh_gradient: bool = False, suspended=None,
                                          suspended_base: str = "identity", device_spectrum: bool = False) -> dict:
    """Objective, constraints and both their gradients for every candidate (``fourier_coefficients`` dicts) -- what ``IpoptProblem.gradient``
    and ``.jacobian`` (optimizer.py:386-416) need, ``compute_analytical_gradient`` for a whole batch -- without a sample leaving the device:
    one ``candidate_states``; ``candidate_objectives`` (f, g, the extrema's indices); the D-optimality gradient
    (``candidate_dopt_gradient_from_coefficients``'s, from the same states and Gram); ``candidate_torque_jacobians`` at the torque peaks; one
    ``Engine.fourier_state_chain`` over the 4 n rows of ``constraint_chain_rows``; ``constraint_gradients_from_rows``; with ``collision``
    the rows of ``candidate_collision_gradient`` at ``layout["collision"]``.  Only per-candidate arrays cross PCIe.

    Returns ``f`` (C,) and ``g`` (C, len), identical to ``candidate_objectives_from_coefficients``; ``obj_grad``: a dict ``wf`` (C,),
    ``q_offset`` / ``q_range`` (C, n), ``a`` / ``b`` (C, n, nh) (the format of ``candidate_dopt_gradient_from_coefficients``), the
    D-optimality term included; ``dopt_grad`` and ``soft_grad``: its two terms (``dopt_grad`` zeros for ``failed`` candidates, whose
    ``obj_grad`` is the soft-cost gradient only); ``con_grad``: the same dict with a leading constraint axis, ``wf`` (C, len), ... in ``constraint_layout`` order;
    ``layout``; ``ag_cache``; ``objectives``: the whole result of ``candidate_objectives``.  ``gradient_to_optimizer_variables`` /
    ``constraint_gradient_to_optimizer_variables`` map ``{k: v[c] ...}`` of both onto the reference's variable vector.

    ``epsilon``: the forward-difference step of both sweeps, None: ``config.get("analyticalGradientEpsilon", 1e-7)``; ``subsample``: of the
    D-optimality sweep (``analyticalGradientSubsample``).  Deviations from the reference: the wf column is analytic, the torque Jacobians
    are the clean derivative (no carried-over dq_{n-1} + eps), the Coulomb sign and the Stribeck exponent are held at their baseline;
    a ``failed`` candidate gets the soft-cost gradient only.  ``box_gradient=False``: a ``collision`` set with box pairs (world links,
    capsule-less links, ``collisionMode: "box"``) raises ``ValueError``; ``True``: their rows are the reference's central differences of
    the box distance over the same ``epsilon`` (``candidate_collision_gradient``).  ``hull_gradient=False``: a ``collision`` set with hull
    pairs raises ``ValueError``; ``True`` with ``collisionMode: "convex"``: the rows of the hull pairs are the reference's central
    differences of the hull distance over the same ``epsilon`` (``candidate_collision_gradient``).  Not covered:
    gravity-only models (refused).  ``mesh_gradient=False``: a ``collision`` set with triangle meshes (``fullMeshLinks``, ``collisionMode:
    "full"``) is refused by the names of the meshed links; ``True`` with such a set and configuration: the rows of all its pairs come from
    ``Engine.mesh_distance_gradients`` (``candidate_collision_gradient``).  ``large_hull_gradient=False``: a ``collision`` set with a hull
    above 128 vertices is refused by the names and vertex counts of those hulls; ``True`` with ``collisionMode: "convex"``, hull pairs only
    and no meshes: the rows of all its pairs come from ``Engine.large_hull_distance_gradients`` (``candidate_collision_gradient``).
    ``large_mesh_gradient=False``: a ``collision`` set built with ``large_meshes=True`` is refused by the names and triangle counts of its
    meshes; ``True`` with such a set of hull pairs only, in ``collisionMode: "full"`` or with ``fullMeshLinks`` in ``"convex"``: the rows
    of all its pairs come from ``Engine.large_mesh_distance_gradients`` (``candidate_collision_gradient``).

    ``suspended`` (``suspended_spec``; floating base only): ``floatingBaseAttachment: "suspended"`` is accepted -- the one
    ``candidate_states(..., suspended=)`` simulates the base motion of every candidate on the device, f and g are those of
    ``candidate_objectives_from_coefficients(..., suspended=)``, every part is the stand-alone entry point's with the same arguments, and
    the result carries ``suspended_info`` (C, 2) int64: the equilibrium iterations and clamp events of
    ``Engine.suspended_base_motion(..., with_info=True)``, so a caller sees that a candidate's base hit the +-25 degree clamp.
    ``suspended_base``: ``"identity"`` (default, the reference's rule) -- the D-optimality weights, the extrema, their indices and
    ``sign_n`` come from the swung states, the D-optimality sweep and the torque sensitivities run at rpy = base_vel = base_acc = 0;
    ``"held"`` -- both sweeps run at the swung states, the partial derivative with the simulated base trajectory frozen.  The collision
    rows hold the base at the pose of the winning evaluation under both (``candidate_collision_gradient``).  Neither rule differentiates
    the base motion (the coupling through the base dynamics is neglected, as in the reference), so a clamp event does not invalidate a
    row: it only says that the frozen trajectory has a kink there.  None: the stationary base, and that configuration is refused.

    ``device_spectrum=True``: the D-optimality terms and the matrices C of the weight rows come from ONE ``Engine.dopt_terms(...,
    weights=True)`` on the Grams in HBM, C scaled by ``dopt_scale`` where it lies: neither the Grams nor C cross PCIe; a candidate whose
    Gram is not finite then raises ``np.linalg.LinAlgError`` (``Engine.dopt_terms``).  False (default):
    the host route, every array as before.  The keyword with ``useBasisProjection`` in ``config`` raises."""
    rest = _suspended_rule(suspended, suspended_base)
    _check_config(config, suspended)
    if device_spectrum:
        _refuse_basis_projection(config)
    if large_mesh_gradient and collision is None:
        raise ValueError("large_mesh_gradient=True: no collision set (collision=)")
    tree_rows = collision is not None and _wants_large_mesh_gradient(config, collision, large_mesh_gradient)
    if not tree_rows:
        _refuse_large_mesh_gradient(collision)
    large_rows = not tree_rows and collision is not None and _wants_large_hull_gradient(config, collision, large_hull_gradient)
    if large_hull_gradient and collision is None:
        raise ValueError("large_hull_gradient=True: no collision set (collision=)")
    if not (large_rows or tree_rows):
        _refuse_large_hull_gradient(collision)
    mesh_rows = not (large_rows or tree_rows) and collision is not None and _wants_mesh_gradient(config, collision, mesh_gradient)
    if not (mesh_rows or tree_rows):
        _refuse_mesh_gradient(collision)
    hull_rows = not (mesh_rows or large_rows or tree_rows) and collision is not None and _wants_hull_gradient(config, collision, hull_gradient)
    if _has_hull_pairs(collision) and not (hull_rows or mesh_rows or large_rows or tree_rows):
        raise ValueError(_NO_HULL_GRADIENT)
    if _has_box_pairs(collision) and not box_gradient:
        raise ValueError("gradients on the device cover capsule pairs only: the collision set has box pairs (the reference differentiates those "
                         "by central differences; box_gradient=True does the same on the device)")
    x_std = getattr(model_or_x_std, "xStdModel", model_or_x_std)
    C, n, T = len(candidates), engine.n, int(T)
    eps = float(config.get("analyticalGradientEpsilon", 1e-7) if epsilon is None else epsilon)
    st = _coefficient_states(engine, candidates, T, freq, config.get("frictionSignThreshold", 0.02), suspended, with_info=suspended is not None)
    info = st.pop("suspended_info", None)
    vel_sign = st["dq"] if getattr(engine, "stribeck", 0.0) > 0 else None
    obj, G, coll, Cm = _candidate_objective_parts(engine, st, C, independent_cols, x_std, limits, joint_names, config, dopt_scale, YtY_prior, vel_sign,
                                                  collision, suspended, device_spectrum, with_weights=device_spectrum)
    ag = obj["ag_cache"]
    dopt = _dopt_gradient(engine, st, G, candidates, T, freq, independent_cols, config.get("doptRegularization", 1e-4), obj["dopt_scale"], YtY_prior,
                          eps, subsample, 2**31, rest_base=rest, weights=None if Cm is None else Cm * obj["dopt_scale"])
    ok = ~obj["failed"]
    dopt = {k: np.where(ok.reshape((C,) + (1,) * (v.ndim - 1)), v, 0.0) for k, v in dopt.items()}
    jac = {k: _host(v) for k, v in candidate_torque_jacobians(engine, st, C, ag["torque_absmax_idx"], x_std, eps, vel_sign=vel_sign,
                                                                rest_base=rest).items()}
    import torch

    vidx = torch.as_tensor(np.asarray(ag["vel_absmax_idx"], dtype=np.int64), device=st["dq"].device).reshape(C, 1, n)
    vel_at_peak = _host(torch.gather(st["dq"].reshape(C, T, n), 1, vidx)[:, 0])
    A, B, nh, qr = _padded_coefficients(candidates, n)
    wf = np.array([c["wf"] for c in candidates], dtype=np.float64)
    chain = lambda smp, gq, gdq, gddq: _host(engine.fourier_state_chain(wf, A, B, smp, float(freq), gq, gdq, gddq, q_range=qr))  # noqa: E731
    pc = constraint_gradients_from_rows(ag, jac, vel_at_peak, chain, limits, joint_names, config, suspended=suspended)
    soft = _gradient_dict(pc["obj_grad"], n, nh)
    con = pc["con_grad"]
    lay = constraint_layout(n, bool(config.get("minVelocityConstraint", False)), None if coll is None else int(np.asarray(coll["g"]).shape[1]))
    con_grad = _gradient_dict(con, n, nh)
    if coll is not None:
        cg = candidate_collision_gradient(engine, st, C, candidates, freq, config, collision, constraints=coll, box_gradient=box_gradient,
                                          epsilon=eps, hull_gradient=hull_rows, mesh_gradient=mesh_rows, large_hull_gradient=large_rows,
                                          large_mesh_gradient=tree_rows, suspended=suspended)["grad"]
        con_grad = {k: np.concatenate([v, cg[k]], axis=1) for k, v in con_grad.items()}
    out = {"f": obj["f"], "g": obj["g"], "obj_grad": {k: dopt[k] + soft[k] for k in soft}, "dopt_grad": dopt, "soft_grad": soft, "con_grad": con_grad,
           "layout": lay, "ag_cache": ag, "objectives": obj}
    if suspended is not None:
        out["suspended_info"] = _host(info)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# The observability analysis of the trajectory file (trajectory.py:225-264) per candidate: which base parameters a candidate does not
# excite and which identified parameters that pins (identifier.py:1536-1562: estimation.merge_unobservable_params).
# ------------------------------------------------------------------------------------------------------------------------------------
def candidate_observability(engine, states: dict, ncand: int, independent_cols, config: dict, w=None, YtY_prior=None) -> dict:
    """The reference's observability analysis of ``ncand`` equal candidates stacked in ``states``: one ``gram_grouped`` and one
    ``Engine.dopt_observability`` on the Gram where it lies -- with device states only per-candidate numbers and one (C, nb) array reach
    the host.  The reference takes an SVD of ``YBase = Y[:, independent_cols]``, counts the singular values below
    ``observabilityThreshold`` (default 1e-6) times the largest, sums the squared components of those right singular vectors per base
    parameter and maps that energy through ``Pb``; here the same numbers come from the eigenpairs of ``YBase^T YBase`` (eigenvalues S^2,
    the same vectors).  Per candidate:

    ``n_observable_base_params`` (C,) int64; ``unobservable_energy`` (C, nb); ``unobservable_params``: a list of C sorted int64 arrays,
    the identified-parameter indices with a score above 0.5 -- ``Pb`` carries the energy of base parameter j to ``independent_cols[j]``
    --; ``observability_threshold``; ``margin`` (C,): the relative distance of the nearest eigenvalue from the cut ``threshold^2
    lambda_max``; ``ambiguous`` (C,) bool: an eigenvalue lies so close to the cut that the fp64 Gram does not decide its side (status
    bit 4); ``status`` (C,).

    The Gram squares the condition number: singular values below about 2e-7 of the largest are not resolved, and a threshold below
    that is refused by the engine.  ``YtY_prior``: the analysis is that of the summed information ``YBase^T YBase + YtY_prior`` (a
    sequential design); the reference has no prior in this step.  A truthy ``useBasisProjection`` in ``config`` raises: the host route
    (an SVD of ``YBase = Y B``) serves that case."""
    _refuse_basis_projection(config, "candidate_observability", "numpy.linalg.svd of YBase = Y B, as trajectory.py does")
    thr = config.get("observabilityThreshold", 1e-6)
    G = engine.gram_grouped(states, int(ncand), w=w)
    o = engine.dopt_observability(G, independent_cols, thr, prior=YtY_prior, device_out=False)
    cols = np.asarray(independent_cols, dtype=np.int64).reshape(-1)
    energy, status = o["energy"], o["status"]
    return {"n_observable_base_params": o["n_observable"], "unobservable_energy": energy,
            "unobservable_params": [np.sort(cols[energy[c] > 0.5]).astype(np.int64) for c in range(energy.shape[0])],
            "observability_threshold": thr, "margin": o["margin"], "ambiguous": (status & 4) != 0, "status": status}


def candidate_observability_from_coefficients(engine, candidates: list, T: int, freq: float, independent_cols, config: dict,
                                              YtY_prior=None) -> dict:
    """``candidate_observability`` from Fourier coefficients (``fourier_coefficients`` dicts): the states are generated on the device
    (``candidate_states``), the Coulomb column of a friction engine is tanh(dq / ``frictionSignThreshold``); neither the samples nor the
    Grams cross PCIe."""
    _refuse_basis_projection(config, "candidate_observability", "numpy.linalg.svd of YBase = Y B, as trajectory.py does")
    st = _coefficient_states(engine, candidates, T, freq, config.get("frictionSignThreshold", 0.02))
    return candidate_observability(engine, st, len(candidates), independent_cols, config, YtY_prior=YtY_prior)


def observability_fields(result: dict, c: int) -> dict:
    """The three keys the reference stores in the trajectory file for candidate ``c`` of a ``candidate_observability`` result, as
    trajectory.py:262-264 writes them: ``unobservable_params`` (an int64 array), ``observability_threshold``,
    ``n_observable_base_params`` (an int) -- ready for ``np.savez(file, **save_dict, **fields)``."""
    return {"unobservable_params": np.array([int(i) for i in result["unobservable_params"][c]], dtype=np.int64),
            "observability_threshold": result["observability_threshold"],
            "n_observable_base_params": int(result["n_observable_base_params"][c])}
