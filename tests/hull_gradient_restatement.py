"""An independent NumPy / Qhull restatement of the hull distance gradient (fbr_hull_distance_gradients): the reference's rule, central
differences of the hull distance over +- eps in EVERY joint, each stencil point a whole re-walk of the robot
(tests/hull_restatement.hull_world) and a Qhull evaluation of the Minkowski difference (hull_restatement.hull_distance) -- deliberately
not the device's formulation, which walks once, moves the hulls rigidly, only for the joints between the two links, and measures them
with GJK and a facet pass.  No code shared with the kernels.

An item is one (candidate, pair): its two hulls are picked from hull_world's frames of the item's own configuration."""
import numpy as np

import hull_restatement as hr
from box_gradient_restatement import path_dofs

EPS = np.finfo(np.float64).eps
NONE = 1e10


def diameters(hulls):
    return np.array([float(np.linalg.norm(h[3][:, None] - h[3][None], axis=2).max()) for h in hulls])


def item_values(topo, hulls, diam, ia, ib, q, floating, rpy, base_pos, offset_in_link_axes, live=None):
    """hull ia[i] against hull ib[i] at configuration q[i]: (dist (M,), pair scale (M,)); ``live`` (M,) bool: the items to evaluate (the
    others NaN)"""
    R, c = hr.hull_world(topo, hulls, q, floating, rpy, base_pos, offset_in_link_axes)
    M = len(q)
    d = np.full(M, np.nan)
    for i in range(M):
        if live is None or live[i]:
            d[i] = hr.hull_distance(R[i, ia[i]], c[i, ia[i]], hulls[ia[i]][3], R[i, ib[i]], c[i, ib[i]], hulls[ib[i]][3])
    rows = np.arange(M)
    return d, hr.pair_scale(c[rows, ia], diam[ia], c[rows, ib], diam[ib])


def evaluate(topo, hulls, pairs, floating, q, rpy, base_pos, C, sample, scale, pose, eps, offset_in_link_axes, dev=None):
    """The contract of fbr_hull_distance_gradients: hulls [(link or -1, offset, rot or None, vertices)], q (C * T, n) [, rpy, base_pos
    (C * T, 3)], sample / scale / pose (C, P) (scale, pose may be None) -> dict of (C, P[, n]) arrays:

    dist, grad        the hull distance at scale * q[sample] and (d+ - d-) / (2 eps) for every joint; 1e10 and a zero row where sample is -1
    dist_p, dist_m    (C, P, n) the distances at the two stencil points
    on_path           (C, P, n) the joints the device evaluates (box_gradient_restatement.path_dofs: the rule is the boxes')
    scale0, scale_p, scale_m   |c_B - c_A| + diam A + diam B at the three stencil points
    bar               (C, P, n) (b+ + b-) / (2 eps), b+- = max(10 dev, 32 EPS scale at the stencil point): the bar of the distances carried
                      through the difference quotient; ``dev``: the largest |g++ emulation - restatement| over the case's centre distances
                      (None: ``bar`` and ``dist_bar`` are left to a later ``with_dev``)
    dist_bar          (C, P) max(10 dev, 32 EPS scale) at the centre

    Asserted (with_dev): the entries of joints off the path are within ``bar`` of 0."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    C, P, n = int(C), pairs.shape[0], topo.num_dofs
    T = q.shape[0] // C
    sample = np.asarray(sample).reshape(C, P)
    pose = sample if pose is None else np.where(np.asarray(pose).reshape(C, P) < 0, sample, np.asarray(pose).reshape(C, P))
    sc = np.ones((C, P)) if scale is None else np.asarray(scale, dtype=np.float64).reshape(C, P)
    base = (np.arange(C) * T)[:, None]
    rq, rp = (base + np.maximum(sample, 0)).reshape(-1), (base + np.maximum(pose, 0)).reshape(-1)
    q0 = q[rq] * sc.reshape(-1, 1)
    r0 = None if rpy is None or not floating else rpy[rp]
    b0 = None if base_pos is None or not floating else base_pos[rp]
    ia, ib = np.tile(pairs[:, 0], C), np.tile(pairs[:, 1], C)
    M = C * P
    live = (sample >= 0).reshape(-1)
    diam = diameters(hulls)
    at = lambda qq: item_values(topo, hulls, diam, ia, ib, qq, floating, r0, b0, offset_in_link_axes, live)  # noqa: E731
    dist, s0 = at(q0)
    grad, sp, sm, dp, dm = (np.zeros((M, n)) for _ in range(5))
    for d in range(n):
        e = np.zeros(n)
        e[d] = eps
        dp[:, d], sp[:, d] = at(q0 + e)
        dm[:, d], sm[:, d] = at(q0 - e)
        grad[:, d] = (dp[:, d] - dm[:, d]) / (2 * eps)
    on = np.zeros((P, n), dtype=bool)
    for k, (a, b) in enumerate(pairs):
        on[k] = path_dofs(topo, hulls[a][0], hulls[b][0], bool(offset_in_link_axes))
    none = sample < 0
    out = {"dist": np.where(none, NONE, dist.reshape(C, P)), "grad": np.where(none[..., None], 0.0, grad.reshape(C, P, n)),
           "dist_p": dp.reshape(C, P, n), "dist_m": dm.reshape(C, P, n), "on_path": np.broadcast_to(on, (C, P, n)).copy(), "scale0": s0.reshape(C, P),
           "scale_p": sp.reshape(C, P, n), "scale_m": sm.reshape(C, P, n), "eps": eps, "none": none}
    return out if dev is None else with_dev(out, dev)


def with_dev(ref, dev):
    """``ref`` with ``bar`` and ``dist_bar`` for the deviation ``dev`` of the emulation's centre distances, and the assertion on the
    off-path entries"""
    out = dict(ref)
    fix = lambda s: np.where(np.isfinite(s), s, 1.0)  # noqa: E731
    bp, bm = np.maximum(10.0 * dev, 32.0 * EPS * fix(ref["scale_p"])), np.maximum(10.0 * dev, 32.0 * EPS * fix(ref["scale_m"]))
    out["bar"] = (bp + bm) / (2.0 * ref["eps"])
    out["dist_bar"] = np.maximum(10.0 * dev, 32.0 * EPS * fix(ref["scale0"]))
    off = ~ref["on_path"] & np.isfinite(ref["grad"])
    assert np.all(np.abs(ref["grad"])[off] <= out["bar"][off]), "an off-path entry of the restatement is not within its bar of 0"
    return out


def separated(ref):
    """(C, P, n) bool: the three distances of the entry's stencil are all positive (the separated distance is C1: no facet switches)"""
    return (ref["dist"][..., None] > 0) & (ref["dist_p"] > 0) & (ref["dist_m"] > 0) & ~ref["none"][..., None]
