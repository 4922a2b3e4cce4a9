"""The collision cases of tests/test_gpu_suspended_gradients.py: the left arm hanging from LShy (problem 0 of
tests/test_suspended_gradient_host.py) with world geometry, so that the pose of the swinging base matters, and NumPy stand-ins for the
engine's distance calls (box_restatement) through which excitation._collision_constraints runs on the host -- the conditions the device test
relies on (a world pair won on the trajectory, one won by a transition configuration at a pose other than sample 0's) are found and checked
with these on the CPU."""
import numpy as np

import box_restatement as br
from test_boxes import synthetic_boxes

BOX_SEED = 3
CONFIG = {"collisionMode": "box", "collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 4, "analyticalGradientEpsilon": 1e-7}


class HostBoxEngine:
    """``candidate_box_distances`` of a floating engine from the restatement: what excitation._collision_constraints needs of an engine"""
    floating = True

    def __init__(self, topo, boxes, pairs, link_axes=False):
        self.topo, self.boxes, self.pairs, self.link_axes = topo, boxes, np.asarray(pairs).reshape(-1, 2), link_axes

    def candidate_box_distances(self, st, C, step, base_pos=None):
        q = np.asarray(st["q"])
        T = q.shape[0] // C
        R, c, h = br.box_world(self.topo, self.boxes, q, True, np.asarray(st["rpy"]), None if base_pos is None else np.asarray(base_pos), self.link_axes)
        d = br.pair_distances(R, c, h, self.pairs)[0].reshape(C, T, -1)[:, ::step]
        k = d.argmin(1)
        return {"dist": np.take_along_axis(d, k[:, None], 1)[:, 0], "idx": k * step}


def box_case(topo, q, rpy, bpos, C, seed=BOX_SEED):
    """Boxes on every link of ``topo`` and three world boxes beside the swinging arm: one near a link at a sample of the trajectory, two near
    links of the arm on its way to the zero posture (0.5 q[0] and 0.5 q[T - 1], at the pose of the largest swing).  Returns the collision
    set of collisionMode "box" (every robot box against every world box, and the robot pairs that are not neighbours)."""
    from test_boxes import mixed_pairs, random_rotations

    rng = np.random.default_rng(seed)
    T = q.shape[0] // C
    boxes = synthetic_boxes(topo, rng)
    ext = int(np.abs(rpy[:T]).sum(1).argmax())
    spots = [(q[T // 2], rpy[T // 2], bpos[T // 2]), (0.5 * q[0], rpy[ext], bpos[ext]), (0.5 * q[2 * T - 1], rpy[T + ext], bpos[T + ext])]
    L = topo.num_links
    for qs, r, b in spots:
        _, p = br.link_poses(topo, qs[None], True, r[None], b[None])
        centre = p[int(rng.integers(L // 2, L))][0] + rng.standard_normal(3) * 0.05 + np.array([0.0, 0.0, -0.25])
        boxes.append((-1, rng.uniform(0.05, 0.15, 3), centre, random_rotations(rng, 1)[0]))
    pairs = mixed_pairs(topo, boxes)
    P = len(pairs)
    return {"boxes": boxes, "box_pairs": pairs, "columns": np.stack([np.ones(P, dtype=np.int64), np.arange(P)], axis=1), "margins": np.zeros(P),
            "center_in_link_axes": False, "capsules": [], "pairs": np.zeros((0, 2), dtype=np.int32)}


MESH_CONFIG = dict(CONFIG, collisionMode="convex")


def mesh_case(topo, q, rpy, bpos, C, seed=BOX_SEED, plain_pairs=3):
    """The hull set over the boxes of ``box_case`` (tests/test_hull_gradient.small_hull, the three kinds in turn) with ONE small mesh -- a
    closed tetrahedron on the last link, inside a hull of its own (tests/test_mesh_gradient.hull_around): every pair with a world hull or the
    meshed hull, and ``plain_pairs`` robot pairs without either.  Returns (collision set with ``meshes``, its configuration with
    ``fullMeshLinks``, (P,) bool: the pair has a world hull)."""
    from test_hull_gradient import small_hull
    from test_mesh_gradient import hull_around, mesh_shape

    box = box_case(topo, q, rpy, bpos, C, seed)
    rng = np.random.default_rng(100 + seed)
    hulls = [small_hull(rng, i % 3, topo.link_names[l] if l >= 0 else None, h, c, R, None if l >= 0 else f"world{i}") for i, (l, h, c, R) in enumerate(box["boxes"])]
    m = max(i for i, b in enumerate(box["boxes"]) if b[0] >= 0)
    half = 0.5 * (hulls[m].vertices.max(0) - hulls[m].vertices.min(0))
    tris = mesh_shape(rng, "tetra", half)
    hulls[m] = hull_around(hulls[m].link_name, tris, hulls[m].offset, 0.1 * float(half.min()))
    world = np.array([b[0] < 0 for b in box["boxes"]])
    pairs = np.asarray(box["box_pairs"])
    special = world[pairs[:, 0]] | world[pairs[:, 1]] | (pairs == m).any(1)
    keep = np.sort(np.concatenate([np.nonzero(special)[0], np.nonzero(~special)[0][:plain_pairs]]))
    pairs = np.ascontiguousarray(pairs[keep])
    P = len(pairs)
    cs = {"hulls": hulls, "hull_pairs": pairs, "columns": np.stack([np.full(P, 2, dtype=np.int64), np.arange(P)], axis=1), "margins": np.zeros(P),
          "offset_in_link_axes": False, "meshes": {m: tris}, "capsules": [], "pairs": np.zeros((0, 2), dtype=np.int32), "box_pairs": []}
    return cs, dict(MESH_CONFIG, fullMeshLinks=[hulls[m].link_name]), world[pairs[:, 0]] | world[pairs[:, 1]]


def world_pairs(cs):
    return np.array([cs["boxes"][a][0] < 0 or cs["boxes"][b][0] < 0 for a, b in np.asarray(cs["box_pairs"])])


def host_constraints(topo, cs, st, C, config=CONFIG):
    """excitation._collision_constraints on the host through HostBoxEngine"""
    from flobaroid_amd import excitation as exc

    eng = HostBoxEngine(topo, cs["boxes"], cs["box_pairs"], bool(cs.get("center_in_link_axes", False)))
    return exc._collision_constraints(eng, eng.candidate_box_distances, st, C, config, cs["margins"])
