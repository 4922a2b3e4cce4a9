"""The collision block of the trajectory optimiser's objective (excitation/trajectoryOptimizer.py objectiveFunc, "check collision
constraints" up to ``self.last_g = g``) with world links and box pairs, restated for ONE candidate as the plain loop it is: every checked
configuration in the reference's order, every pair of ``_collision_pairs`` -- the capsule routine when both links have a capsule (capsule
mode), the box routine otherwise --, ``d - margin < g``.  Also ``_buildCollisionPairs`` line by line.  Distances from
tests/capsule_restatement.py and tests/box_restatement.py, one configuration at a time."""
import numpy as np

import box_restatement as br
from capsule_restatement import capsule_distances, capsule_world
from collision_restatement import transition_configs


def build_collision_pairs(link_names, world_links, neighbors, config, no_geometry_links):
    """``_buildCollisionPairs``: (pairs, margins)"""
    all_links = list(link_names) + list(world_links)
    ignore_links = set(config.get("ignoreLinksForCollision", [])) | set(no_geometry_links)
    ignore_pairs = {(a, b) for a, b in config.get("ignoreLinkPairsForCollision", [])} | {(b, a) for a, b in config.get("ignoreLinkPairsForCollision", [])}
    max_kin_dist = config.get("collisionMaxKinematicDistance", 0)

    def _kin_distance(start, target):
        visited = {start}
        queue = [(start, 0)]
        while queue:
            current, dist = queue.pop(0)
            if current == target:
                return dist
            for nb in neighbors.get(current, []):
                if nb not in visited:
                    visited.add(nb)
                    queue.append((nb, dist + 1))
        return 999

    group_ignore = set()
    for group_pair in config.get("ignoreCollisionBetweenGroups", []):
        if len(group_pair) == 2:
            for a in group_pair[0]:
                for b in group_pair[1]:
                    group_ignore.add((a, b))
                    group_ignore.add((b, a))
    pairs = []
    num_robot_links = len(link_names)
    for l0 in range(len(all_links)):
        for l1 in range(l0 + 1, len(all_links)):
            l0_name, l1_name = all_links[l0], all_links[l1]
            if l0 >= num_robot_links and l1 >= num_robot_links:
                continue
            if l0_name in ignore_links or l1_name in ignore_links:
                continue
            if (l0_name, l1_name) in ignore_pairs:
                continue
            if (l0_name, l1_name) in group_ignore:
                continue
            if l0 < num_robot_links and l1 < num_robot_links:
                if l0_name in neighbors[l1_name] or l1_name in neighbors[l0_name]:
                    continue
            if max_kin_dist > 0 and _kin_distance(l0_name, l1_name) > max_kin_dist:
                continue
            pairs.append((l0_name, l1_name))
    world_margin = float(config.get("worldCollisionMargin", 0.0))
    world_link_set = set(world_links)
    margins = np.array([world_margin if (l0 in world_link_set or l1 in world_link_set) else 0.0 for l0, l1 in pairs])
    return pairs, margins


def index_boxes(topo, boxes):
    """collision.Box objects -> the tuples of box_restatement: (link index or -1, half, centre, rot)"""
    names = list(topo.link_names)
    return [(-1 if b.link_name is None else names.index(b.link_name), b.half, b.center, b.rot) for b in boxes]


def config_distances(topo, floating, cs, q, rpy, base_pos):
    """the distances (P,) of every pair of ``cs["pair_names"]`` at ONE configuration, each from the routine the reference sends it to"""
    names = list(topo.link_names)
    cols = np.asarray(cs["columns"])
    d = np.empty(len(cols))
    r = None if rpy is None else rpy[None]
    b = None if base_pos is None else base_pos[None]
    cap = cols[:, 0] == 0
    if cap.any():
        caps = [(names.index(c.link_name), c.p0_local, c.p1_local, c.radius) for c in cs["capsules"]]
        d[cap] = capsule_distances(capsule_world(topo, caps, q[None], floating, r, b), caps, cs["pairs"])["dist"][0][cols[cap, 1]]
    if (~cap).any():
        R, c, h = br.box_world(topo, index_boxes(topo, cs["boxes"]), q[None], floating, r, b, bool(cs.get("center_in_link_axes", False)))
        d[~cap] = br.pair_distances(R, c, h, cs["box_pairs"])[0][0][cols[~cap, 1]]
    return d


def restate_mixed_block(topo, floating, cs, pos, config, rpy=None, base_pos=None):
    """(g (P,), argmin {pair: sample index}, all main-trajectory distances (Tc, P)) of one candidate"""
    T = pos.shape[0]
    rpy = np.zeros((T, 3)) if rpy is None else rpy
    step = config.get("collisionCheckStep", 3)
    configs = [(p, pos[p], rpy[p], None if base_pos is None else base_pos[p]) for p in range(0, T, step)]
    configs += transition_configs(pos, rpy, base_pos, config)
    margins = cs["margins"]
    P = len(cs["pair_names"])
    g = np.full(P, 1e10)
    argmin = {}
    main = []
    for p_idx, q, r, b in configs:
        d = config_distances(topo, floating, cs, q, r, b)
        if p_idx >= 0:
            main.append(d)
        for k in range(P):
            dk = d[k] - margins[k]
            if dk < g[k]:
                g[k] = dk
                if p_idx >= 0:
                    argmin[k] = p_idx
    return g, argmin, np.array(main)
