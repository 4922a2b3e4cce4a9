"""An independent restatement of the trajectory optimiser's objective (excitation/trajectoryOptimizer.py objectiveFunc, the part after the
D-optimality term, without the collision constraints) for ONE candidate, written from the reference's definitions as a plain per-joint
loop -- what the tests hold excitation.objectives_from_extrema and the device extrema against."""
import numpy as np


def restate_objective(neg_log_det, ext, limits, joint_names, config, dopt_scale):
    """``ext``: the candidate's extrema (n,) each: q_min, q_max, dq_absmax, tau_absmax."""
    n = len(joint_names)
    minvel = bool(config.get("minVelocityConstraint", False))
    g = []
    lower_blk, upper_blk, vel_blk, tau_blk, minvel_blk, util_blk = [], [], [], [], [], []
    ovr = config.get("ovrPosLimit", {})
    for i, j in enumerate(joint_names):
        lim = limits[j]
        pair = ovr.get(j) if isinstance(ovr, dict) else None
        lo = np.deg2rad(pair[0]) if pair else lim["lower"]
        hi = np.deg2rad(pair[1]) if pair else lim["upper"]
        lower_blk.append(lo - ext["q_min"][i])
        upper_blk.append(ext["q_max"][i] - hi)
        vel_blk.append(ext["dq_absmax"][i] - lim["velocity"])
        tau_blk.append(ext["tau_absmax"][i] - lim["torque"])
        if minvel:
            minvel_blk.append(lim["velocity"] * config["minVelocityPercentage"] - ext["dq_absmax"][i])
        util_blk.append(lim["torque"] * config.get("minTorqueUtilization", 0.02) - ext["tau_absmax"][i])
    g = np.array(lower_blk + upper_blk + vel_blk + tau_blk + minvel_blk + util_blk, dtype=float)
    g = np.where(np.isnan(g), 10.0, g)

    dopt = neg_log_det * dopt_scale
    f = dopt
    failed = False
    if not np.isfinite(f):
        f, failed = 100.0, True
    util = [ext["tau_absmax"][i] / limits[j]["torque"] for i, j in enumerate(joint_names)]
    mean = sum(util) / n
    std = (sum((u - mean) ** 2 for u in util) / n) ** 0.5
    f1 = std / mean if mean > 0 else 1.0
    f3 = max(0.0, 1.0 - mean / config.get("trajectoryTargetTorqueUtil", 0.25))
    prange = [(ext["q_max"][i] - ext["q_min"][i]) / (limits[j]["upper"] - limits[j]["lower"]) for i, j in enumerate(joint_names)]
    f2 = (1.0 - sum(prange) / n) * 10.0
    vt = float(config.get("trajectoryTargetVelocity", 0.0))
    f4 = sum(max(0.0, 1.0 - ext["dq_absmax"][i] / vt) for i in range(n)) / n if vt > 0 else 0.0
    f = f + 10.0 * f1 + 10.0 * f3 + f2 + 10.0 * f4
    return {"f": f, "g": g, "dopt": dopt, "f1": f1, "f2": f2, "f3": f3, "f4": f4, "failed": failed}


def restate_from_samples(neg_log_det, pos, vel, torques, fb, limits, joint_names, config, dopt_scale):
    """The same from a candidate's samples: positions / velocities (T, n), torques (T, fb + n) as computeRegressors hands them on
    (np.nan_to_num of the simulated torques); the extrema taken as objectiveFunc takes them."""
    tq = np.nan_to_num(torques)
    ext = {"q_min": np.min(pos, axis=0), "q_max": np.max(pos, axis=0), "dq_absmax": np.max(np.abs(vel), axis=0),
           "tau_absmax": np.nanmax(np.abs(tq[:, fb:]), axis=0)}
    out = restate_objective(neg_log_det, ext, limits, joint_names, config, dopt_scale)
    out["idx"] = {"torque_absmax_idx": np.argmax(np.abs(tq[:, fb:]), axis=0), "pos_min_idx": np.argmin(pos, axis=0),
                  "pos_max_idx": np.argmax(pos, axis=0), "vel_absmax_idx": np.argmax(np.abs(vel), axis=0)}
    return out
