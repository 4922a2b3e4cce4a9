"""An independent NumPy / Qhull restatement of the mesh distance gradient (fbr_mesh_distance_gradients): the reference's rule, central
differences over +- eps in EVERY joint, each stencil point a whole re-walk of the robot (tests/hull_restatement.hull_world) and the mesh
distance of tests/mesh_restatement.py -- triangle against hull through Qhull, clamped at 0, triangle against triangle in closed form; a
pair without a mesh the signed hull distance of tests/hull_restatement.py.  Deliberately not the device's formulation, which walks once,
records the relative poses of the evaluated joints' stencil points and measures each with GJK in a wave of its own.  No code shared with
the kernels.

This is tests/hull_gradient_restatement.evaluate with the item distance replaced; its ``with_dev`` (the bars and the assertion on the
off-path entries) is used as it is."""
import numpy as np

import hull_gradient_restatement as hg
import hull_restatement as hr
import mesh_restatement as mr
from box_gradient_restatement import path_dofs

EPS = hg.EPS
NONE = hg.NONE


def with_dev(ref, dev):
    """hull_gradient_restatement.with_dev (``bar``, ``dist_bar``, the assertion on the off-path entries), and ``dev`` itself"""
    return dict(hg.with_dev(ref, dev), dev=float(dev))


def item_values(topo, hulls, meshes, diam, ia, ib, q, floating, rpy, base_pos, offset_in_link_axes, live=None):
    """hull ia[i] against hull ib[i] at configuration q[i], either with its mesh when it has one: (signed value (M,), pair scale (M,));
    ``live`` (M,) bool: the items to evaluate (the others NaN)"""
    R, c = hr.hull_world(topo, hulls, q, floating, rpy, base_pos, offset_in_link_axes)
    M = len(q)
    d = np.full(M, np.nan)
    for i in range(M):
        if live is None or live[i]:
            a, b = int(ia[i]), int(ib[i])
            if a in meshes or b in meshes:
                d[i] = mr.mesh_signed(R[i, a], c[i, a], meshes.get(a), hulls[a][3], R[i, b], c[i, b], meshes.get(b), hulls[b][3])
            else:
                d[i] = hr.hull_distance(R[i, a], c[i, a], hulls[a][3], R[i, b], c[i, b], hulls[b][3])
    rows = np.arange(M)
    return d, hr.pair_scale(c[rows, ia], diam[ia], c[rows, ib], diam[ib])


def evaluate(topo, hulls, meshes, pairs, floating, q, rpy, base_pos, C, sample, scale, pose, eps, offset_in_link_axes, dev=None):
    """The contract of fbr_mesh_distance_gradients: hulls [(link or -1, offset, rot or None, vertices)], meshes {hull index: (T, 3, 3)}, the
    other arguments as hull_gradient_restatement.evaluate -> its dict, the distances of pairs with a mesh clamped at 0, and

    meshed                       (P,) bool: the pair has a mesh on either side
    signed0, signed_p, signed_m  the restatement's signed values at the three stencil points ((C, P), (C, P, n), (C, P, n)): negative where
                                 the geometries intersect -- how clear the verdict "gap" or "contact" is"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    meshes = {int(h): np.asarray(t, dtype=np.float64).reshape(-1, 3, 3) for h, t in dict(meshes).items()}
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
    diam = hg.diameters(hulls)
    meshed = np.array([int(a) in meshes or int(b) in meshes for a, b in pairs])
    mm = np.tile(meshed, C)
    value = lambda s: np.where(mm, mr.clamp(s), s)  # noqa: E731
    at = lambda qq: item_values(topo, hulls, meshes, diam, ia, ib, qq, floating, r0, b0, offset_in_link_axes, live)  # noqa: E731
    sg0, s0 = at(q0)
    grad, sp, sm, gp, gm = (np.zeros((M, n)) for _ in range(5))
    for d in range(n):
        e = np.zeros(n)
        e[d] = eps
        gp[:, d], sp[:, d] = at(q0 + e)
        gm[:, d], sm[:, d] = at(q0 - e)
        grad[:, d] = (value(gp[:, d]) - value(gm[:, d])) / (2 * eps)
    on = np.zeros((P, n), dtype=bool)
    for k, (a, b) in enumerate(pairs):
        on[k] = path_dofs(topo, hulls[a][0], hulls[b][0], bool(offset_in_link_axes))
    none = sample < 0
    m2 = mm[:, None]
    out = {"dist": np.where(none, NONE, value(sg0).reshape(C, P)), "grad": np.where(none[..., None], 0.0, grad.reshape(C, P, n)),
           "dist_p": np.where(m2, mr.clamp(gp), gp).reshape(C, P, n), "dist_m": np.where(m2, mr.clamp(gm), gm).reshape(C, P, n),
           "on_path": np.broadcast_to(on, (C, P, n)).copy(), "scale0": s0.reshape(C, P), "scale_p": sp.reshape(C, P, n), "scale_m": sm.reshape(C, P, n),
           "eps": eps, "none": none, "meshed": meshed, "signed0": sg0.reshape(C, P), "signed_p": gp.reshape(C, P, n), "signed_m": gm.reshape(C, P, n)}
    return out if dev is None else with_dev(out, dev)


def clear_verdicts(ref):
    """(C, P) bool: at the centre and at the two stencil points of every evaluated joint the signed value of a pair with a mesh is more
    than 100 of that point's distance bars from 0 -- a clear gap or a clear intersection (the rule of tests/test_meshes.py); pairs without
    a mesh and items without a sample are clear by definition.  Needs ``with_dev``."""
    fix = lambda s: np.where(np.isfinite(s), s, 1.0)  # noqa: E731
    bp, bm = (np.maximum(10.0 * ref["dev"], 32.0 * EPS * fix(ref[k])) for k in ("scale_p", "scale_m"))
    ok0 = np.abs(fix(ref["signed0"])) > 100.0 * ref["dist_bar"]
    okp = (np.abs(fix(ref["signed_p"])) > 100.0 * bp) & (np.abs(fix(ref["signed_m"])) > 100.0 * bm)
    ok = ok0 & np.where(ref["on_path"], okp, True).all(axis=2)
    return ok | ~ref["meshed"][None, :] | ref["none"]
