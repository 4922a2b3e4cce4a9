"""The collision block of the trajectory optimiser's objective (excitation/trajectoryOptimizer.py objectiveFunc, "check collision
constraints" up to ``self.last_g = g``, capsule mode) restated for ONE candidate as the plain loop it is: every checked configuration in
the reference's order, every pair, ``d - margin < g``.  Distances from tests/capsule_restatement.py, one configuration at a time."""
import numpy as np

from capsule_restatement import capsule_distances, capsule_world


def transition_configs(pos, rpy, base_pos, config):
    """[(index, q, rpy, base_pos)] of the minimum-jerk ramps from / to the zero position, numbered -1, -2, ... as the reference does."""
    out = []
    if config.get("transitionDuration", 3.0) <= 0:
        return out
    ns = config.get("transitionCollisionSamples", 10)
    idx = list(np.linspace(0, len(rpy) - 1, 6).astype(int))
    idx.append(int(np.argmax(np.abs(rpy).sum(axis=1))))
    poses = [(rpy[i], None if base_pos is None else base_pos[i]) for i in sorted(set(idx))]
    count = 0
    for qb in (pos[0], pos[-1]):
        for ti in range(ns):
            tau = (ti + 1) / (ns + 1)
            s = 10.0 * tau**3 - 15.0 * tau**4 + 6.0 * tau**5
            for r, b in poses:
                count += 1
                out.append((-count, np.zeros(pos.shape[1]) + s * (qb - np.zeros(pos.shape[1])), r, b))
    return out


def restate_collision_block(topo, floating, capsules, pairs, margins, pos, config, rpy=None, base_pos=None):
    """(g (P,), argmin {pair: sample index}) of one candidate: pos (T, n), rpy (T, 3) (None: zeros, as computeTrajectoryDynamics sets
    it), base_pos (T, 3) or None."""
    T = pos.shape[0]
    rpy = np.zeros((T, 3)) if rpy is None else rpy
    step = config.get("collisionCheckStep", 3)
    configs = [(p, pos[p], rpy[p], None if base_pos is None else base_pos[p]) for p in range(0, T, step)]
    configs += transition_configs(pos, rpy, base_pos, config)
    P = len(pairs)
    g = np.full(P, 1e10)
    argmin = {}
    for p_idx, q, r, b in configs:
        ep = capsule_world(topo, capsules, q[None], floating, r[None], None if b is None else b[None])
        d = capsule_distances(ep, capsules, pairs)["dist"][0]
        for k in range(P):
            dk = d[k] - margins[k]
            if dk < g[k]:
                g[k] = dk
                if p_idx >= 0:
                    argmin[k] = p_idx
    return g, argmin
