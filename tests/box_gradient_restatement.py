"""An independent NumPy restatement of the box distance gradient (fbr_box_distance_gradients): the reference's rule, central differences
of the box distance over +- eps in EVERY joint, each stencil point a whole re-walk of the robot (tests/box_restatement.box_world on
tests/np_dynamics.world_kinematics) -- deliberately not the device's formulation, which walks once and moves the boxes rigidly, and only
for the joints between the two links.  No code shared with the kernels.

An item is one (candidate, pair); its two boxes are picked from box_world's frames of the item's own configuration and go through
box_restatement.box_distance and pair_scale, the two functions pair_distances is made of (pair_distances itself would evaluate every pair at
every item's configuration)."""
import numpy as np

import box_restatement as br

EPS = np.finfo(np.float64).eps
NONE = 1e10


def chain(topo, l):
    out = []
    while l >= 0:
        out.append(l)
        l = topo.parent[l]
    return out


def path_dofs(topo, la, lb, center_in_link_axes=True):
    """bool (n,): the joints with a variable between links la and lb -- above exactly one of them; lb (or la) -1: a world box, every joint
    above the robot link.  From topo.parent (and the dof a link's joint drives).  With the centre offsets in world axes
    (``center_in_link_axes`` False) a REVOLUTE joint above both links counts too: it turns the links, not the offsets, so the pair does not
    move rigidly and the entry is a true non-zero (measured on kuka: up to 0.12)."""
    ca, cb = set(chain(topo, la)), set(chain(topo, lb))
    on = np.zeros(topo.num_dofs, dtype=bool)
    for l in ca ^ cb:
        if topo.dof_index[l] >= 0:
            on[topo.dof_index[l]] = True
    if not center_in_link_axes:
        for l in ca & cb:
            if topo.dof_index[l] >= 0 and topo.joint_type[l] == 1:
                on[topo.dof_index[l]] = True
    return on


def item_values(topo, boxes, ia, ib, q, floating, rpy, base_pos, center_in_link_axes):
    """box ia[i] against box ib[i] at configuration q[i]: (dist, pair_scale, squared lengths of the 9 cross axes, SAT gap), (M, ...) each"""
    R, c, h = br.box_world(topo, boxes, q, floating, rpy, base_pos, center_in_link_axes)
    rows = np.arange(len(q))
    RA, cA, hA, RB, cB, hB = R[rows, ia], c[rows, ia], h[ia], R[rows, ib], c[rows, ib], h[ib]
    fin = np.isfinite(RA).all((1, 2)) & np.isfinite(RB).all((1, 2)) & np.isfinite(cA).all(1) & np.isfinite(cB).all(1)
    z = lambda x: np.where(fin.reshape((-1,) + (1,) * (x.ndim - 1)), x, 0.0)  # noqa: E731
    gap = np.where(fin, br.sat_gap(z(RA), z(cA), hA, z(RB), z(cB), hB), np.nan)
    return br.box_distance(RA, cA, hA, RB, cB, hB), br.pair_scale(cA, hA, cB, hB), br.sat_axes(z(RA), z(RB))[1], gap


def evaluate(topo, boxes, pairs, floating, q, rpy, base_pos, C, sample, scale, pose, eps, center_in_link_axes, dev=None):
    """The contract of fbr_box_distance_gradients: q (C * T, n) [, rpy, base_pos (C * T, 3)], sample / scale / pose (C, P) (scale, pose may be
    None) -> dict of (C, P[, n]) arrays:

    dist, grad   the box distance at scale * q[sample] and (d+ - d-) / (2 eps) for every joint; 1e10 and a zero row where sample is -1
    on_path      (C, P, n) the joints between the pair's links (path_dofs)
    bar          (C, P, n) (b+ + b-) / (2 eps), b+- = max(10 dev, 32 EPS pair_scale at the stencil point): the bar of the distances
                 (tests/test_gpu_boxes.reference_case) carried through the difference quotient; ``dev``: the largest |g++ emulation -
                 restatement| over the case's distances (None: ``bar`` and ``dist_bar`` are left to a later ``with_dev``)
    dist_bar     (C, P) max(10 dev, 32 EPS pair_scale) at the centre
    gap, gap_p, gap_m   the SAT gap at the centre (C, P) and at the stencil points (C, P, n)

    Asserted here: no |a_i x b_j|^2 of a stencil point lies within a factor 100 of the threshold 1e-12 below which the library skips a
    cross axis; the entries of joints off the path are within ``bar`` of 0."""
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

    def at(qq):
        d, s, len2, gap = item_values(topo, boxes, ia, ib, qq, floating, r0, b0, center_in_link_axes)
        fin = np.isfinite(d) & live
        assert not ((len2[fin] >= br.PARALLEL / 100) & (len2[fin] <= br.PARALLEL * 100)).any(), "a cross axis near the threshold: change the seed"
        return d, s, gap

    dist, s0, gap0 = at(q0)
    grad, sp, sm = np.zeros((M, n)), np.zeros((M, n)), np.zeros((M, n))
    gp, gm = np.zeros((M, n)), np.zeros((M, n))
    for d in range(n):
        e = np.zeros(n)
        e[d] = eps
        dp, sp[:, d], gp[:, d] = at(q0 + e)
        dm, sm[:, d], gm[:, d] = at(q0 - e)
        grad[:, d] = (dp - dm) / (2 * eps)
    on = np.zeros((P, n), dtype=bool)
    for k, (a, b) in enumerate(pairs):
        on[k] = path_dofs(topo, boxes[a][0], boxes[b][0], bool(center_in_link_axes))
    none = sample < 0
    out = {"dist": np.where(none, NONE, dist.reshape(C, P)), "grad": np.where(none[..., None], 0.0, grad.reshape(C, P, n)),
           "on_path": np.broadcast_to(on, (C, P, n)).copy(), "scale0": s0.reshape(C, P), "scale_p": sp.reshape(C, P, n), "scale_m": sm.reshape(C, P, n),
           "gap": gap0.reshape(C, P), "gap_p": gp.reshape(C, P, n), "gap_m": gm.reshape(C, P, n), "eps": eps, "none": none}
    return out if dev is None else with_dev(out, dev)


def with_dev(ref, dev):
    """``ref`` with ``bar`` and ``dist_bar`` for the deviation ``dev`` of the emulation's distances, and the assertion on the off-path
    entries"""
    out = dict(ref)
    fix = lambda s: np.where(np.isfinite(s), s, 1.0)  # noqa: E731
    bp, bm = np.maximum(10.0 * dev, 32.0 * EPS * fix(ref["scale_p"])), np.maximum(10.0 * dev, 32.0 * EPS * fix(ref["scale_m"]))
    out["bar"] = (bp + bm) / (2.0 * ref["eps"])
    out["dist_bar"] = np.maximum(10.0 * dev, 32.0 * EPS * fix(ref["scale0"]))
    off = ~ref["on_path"] & np.isfinite(ref["grad"])
    assert np.all(np.abs(ref["grad"])[off] <= out["bar"][off]), "an off-path entry of the restatement is not within its bar of 0"
    return out


def one_sided(ref):
    """(C, P, n) bool: the SAT gap keeps its sign over the three points of the entry's stencil (the distance has no kink at gap = 0 there)"""
    s0 = np.sign(ref["gap"])[..., None]
    return (np.sign(ref["gap_p"]) == s0) & (np.sign(ref["gap_m"]) == s0) & (s0 != 0)
