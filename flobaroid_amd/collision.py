"""Host side of the capsule collision constraints (the reference's ``collisionMode: "capsule"``): capsules fitted to the collision geometry
of a URDF and the list of link pairs the trajectory optimiser checks.  NumPy and ElementTree only.

* ``fit_capsules_from_urdf`` -- excitation/capsule.py ``fit_capsules_from_urdf`` for ``cylinder``, ``sphere`` and ``box`` geometry and the
  merge of several primitives of one link.  There is no mesh code in this project: a link whose only collision geometry is a mesh gets no
  capsule and is reported (callers may add capsules of their own, e.g. fitted to a bounding box they have).
* ``collision_pairs`` -- excitation/trajectoryOptimizer.py ``_buildCollisionPairs`` for the robot's own links: ``ignoreLinksForCollision``,
  ``ignoreLinkPairsForCollision``, ``ignoreCollisionBetweenGroups``, neighbours skipped, ``collisionMaxKinematicDistance``, in the
  reference's pair order.  World links have no capsules in the reference either (they go to its mesh library): out of scope.
* ``collision_set`` -- both in the form ``Engine.set_capsules`` and the ``collision`` argument of ``excitation.candidate_objectives`` take.

The distances themselves are computed on the device (``Engine.candidate_capsule_distances``, csrc/fbr_capsule.h).
"""
from __future__ import annotations

import xml.etree.ElementTree as ET
from dataclasses import dataclass

import numpy as np


@dataclass
class Capsule:
    """A segment ``p0_local`` -- ``p1_local`` in the frame of link ``link_name`` plus a radius (p0 == p1: a sphere)."""

    link_name: str
    p0_local: np.ndarray
    p1_local: np.ndarray
    radius: float


def _origin(element):
    """<origin xyz rpy> -> (position, rotation matrix); fixed-axis XYZ roll-pitch-yaw."""
    if element is None:
        return np.zeros(3), np.eye(3)
    pos = np.array([float(v) for v in element.attrib.get("xyz", "0 0 0").split()])
    r, p, y = (float(v) for v in element.attrib.get("rpy", "0 0 0").split())
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                  [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                  [-sp, cp * sr, cp * cr]])
    return pos, R


def _from_cylinder(pos, rot, length, radius):
    """a URDF cylinder lies along its local z axis, centred at its origin"""
    half = length / 2.0
    return pos + rot @ np.array([0.0, 0.0, -half]), pos + rot @ np.array([0.0, 0.0, half]), radius


def _from_box(pos, rot, size):
    """a capsule along the longest axis of the box: the radius is the larger of the two shorter half extents, the end points are pulled
    inwards by it (not past the centre) so that the caps end at the faces"""
    k = int(np.argmax(size))
    half = size[k] / 2.0
    direction = np.zeros(3)
    direction[k] = 1.0
    radius = float(np.max(np.delete(size, k)) / 2.0)
    inward = min(radius, half)
    return pos + rot @ (-(half - inward) * direction), pos + rot @ ((half - inward) * direction), radius


def _merge(prims):
    """several primitives of one link -> one capsule between their two most distant end points with the largest radius, the end points
    pulled inwards by that radius when the segment is longer than two radii"""
    if len(prims) == 1:
        return prims[0]
    pts, rmax = [], 0.0
    for p0, p1, r in prims:
        pts += [p0, p1]
        rmax = max(rmax, r)
    pts = np.array(pts)
    best, bi, bj = 0.0, 0, 1
    for i in range(len(pts)):
        for j in range(i + 1, len(pts)):
            d = float(np.linalg.norm(pts[i] - pts[j]))
            if d > best:
                best, bi, bj = d, i, j
    p0, p1 = pts[bi].copy(), pts[bj].copy()
    axis = p1 - p0
    length = float(np.linalg.norm(axis))
    if length > 2.0 * rmax:
        unit = axis / length
        p0 = p0 + rmax * unit
        p1 = p1 - rmax * unit
    return p0, p1, rmax


def fit_capsules_from_urdf(urdf, link_names, radius_scale: float = 1.0):
    """``(capsules, mesh_only)``: ``capsules`` maps the name of every link of ``link_names`` that has ``cylinder`` / ``sphere`` / ``box``
    collision geometry in the URDF file ``urdf`` to its ``Capsule`` (document order; ``radius_scale`` multiplies the radii);
    ``mesh_only`` lists the links whose collision geometry consists of meshes only -- they get no capsule here.  Links without a
    <collision> element appear in neither."""
    tree = ET.parse(urdf)
    wanted = set(link_names)
    capsules: dict[str, Capsule] = {}
    mesh_only: list[str] = []
    for link in tree.findall("link"):
        name = link.attrib["name"]
        if name not in wanted:
            continue
        colls = link.findall("collision")
        if not colls:
            continue
        prims, meshes = [], 0
        for coll in colls:
            pos, rot = _origin(coll.find("origin"))
            geom = coll.find("geometry")
            if geom is None:
                continue
            cyl, sph, box = geom.find("cylinder"), geom.find("sphere"), geom.find("box")
            if cyl is not None:
                prims.append(_from_cylinder(pos, rot, float(cyl.attrib["length"]), float(cyl.attrib["radius"])))
            elif sph is not None:
                prims.append((pos.copy(), pos.copy(), float(sph.attrib["radius"])))
            elif box is not None:
                prims.append(_from_box(pos, rot, np.array([float(v) for v in box.attrib["size"].split()])))
            elif geom.find("mesh") is not None:
                meshes += 1
        if prims:
            p0, p1, r = _merge(prims)
            capsules[name] = Capsule(name, p0, p1, r * radius_scale)
        elif meshes:
            mesh_only.append(name)
    return capsules, mesh_only


def link_neighbors(topology) -> dict:
    """The reference's ``URDFHelpers.getNeighbors(model, connected=True)`` on a ``Topology``: per link the names of the links joined to it
    by a joint, plus every link reached from one of those through fixed joints only."""
    names = list(topology.link_names)
    L = len(names)
    adj: list[list[int]] = [[] for _ in range(L)]
    for l, p in enumerate(topology.parent):
        if p >= 0:
            adj[l].append(p)
            adj[p].append(l)
    fixed = lambda a, b: topology.joint_type[a if topology.parent[a] == b else b] == 0  # noqa: E731 (the joint between two adjacent links)
    out = {}
    for l in range(L):
        nb = list(adj[l])
        i = 0
        while i < len(nb):  # (the list grows while it is walked: chains of fixed joints are followed to their end)
            for x in adj[nb[i]]:
                if fixed(nb[i], x) and x != l and x not in nb:
                    nb.append(x)
            i += 1
        out[names[l]] = [names[x] for x in nb]
    return out


def collision_pairs(topology, capsules, config: dict) -> list:
    """Link pairs ``(l0, l1)`` (names, l0 before l1 in ``topology.link_names``) the optimiser checks, in its order.  Skipped: links
    without a capsule or in ``ignoreLinksForCollision``; pairs in ``ignoreLinkPairsForCollision`` (either order) or across two groups of
    ``ignoreCollisionBetweenGroups``; neighbours (``link_neighbors``); with ``collisionMaxKinematicDistance`` > 0, pairs further apart
    than that many steps of the neighbour graph."""
    names = list(topology.link_names)
    ignore_links = set(config.get("ignoreLinksForCollision", [])) | {n for n in names if n not in capsules}
    ignore_pairs = set()
    for a, b in config.get("ignoreLinkPairsForCollision", []):
        ignore_pairs |= {(a, b), (b, a)}
    group_ignore = set()
    for gp in config.get("ignoreCollisionBetweenGroups", []):
        if len(gp) == 2:
            for a in gp[0]:
                for b in gp[1]:
                    group_ignore |= {(a, b), (b, a)}
    nbs = link_neighbors(topology)
    max_dist = config.get("collisionMaxKinematicDistance", 0)

    def kin_distance(start, target):
        seen, queue = {start}, [(start, 0)]
        while queue:
            cur, d = queue.pop(0)
            if cur == target:
                return d
            for x in nbs.get(cur, []):
                if x not in seen:
                    seen.add(x)
                    queue.append((x, d + 1))
        return 999

    pairs = []
    for i, l0 in enumerate(names):
        for l1 in names[i + 1:]:
            if l0 in ignore_links or l1 in ignore_links:
                continue
            if (l0, l1) in ignore_pairs or (l0, l1) in group_ignore:
                continue
            if l0 in nbs[l1] or l1 in nbs[l0]:
                continue
            if max_dist > 0 and kin_distance(l0, l1) > max_dist:
                continue
            pairs.append((l0, l1))
    return pairs


def collision_set(topology, capsules, config: dict, margins=None) -> dict:
    """What ``Engine.set_capsules`` and the ``collision`` argument of ``excitation.candidate_objectives`` take: ``capsules`` (a list, one per
    link that has one, in link order), ``pairs`` ((P, 2) indices into that list, from ``collision_pairs``), ``pair_names`` and ``margins``
    ((P,), default 0: the reference's ``_collision_pair_margins`` are zero for pairs of robot links)."""
    names = [n for n in topology.link_names if n in capsules]
    pos = {n: i for i, n in enumerate(names)}
    pair_names = collision_pairs(topology, capsules, config)
    pairs = np.array([(pos[a], pos[b]) for a, b in pair_names], dtype=np.int32).reshape(-1, 2)
    m = np.zeros(len(pair_names)) if margins is None else np.asarray(margins, dtype=np.float64).reshape(len(pair_names))
    return {"capsules": [capsules[n] for n in names], "pairs": pairs, "pair_names": pair_names, "margins": m}
