"""Host side of the collision constraints (the reference's ``collisionMode: "capsule"``, ``"box"``, ``"convex"`` and ``"full"``, and its
``fullMeshLinks``; robot and world links): capsules, boxes, convex hulls and triangle meshes from the collision geometry of a URDF, the boxes
of a world URDF, and the list of link pairs the trajectory optimiser checks.  NumPy and ElementTree; the hulls come from ``scipy.spatial.ConvexHull`` and a built-in STL reader (no trimesh, no FCL).

* ``fit_capsules_from_urdf`` -- excitation/capsule.py ``fit_capsules_from_urdf`` for ``cylinder``, ``sphere`` and ``box`` geometry and the
  merge of several primitives of one link.  No capsule is fitted to a mesh: a link whose only collision geometry is a mesh gets no
  capsule and is reported (callers may add capsules of their own, e.g. fitted to a bounding box they have).
* ``boxes_from_hulls`` / ``boxes_from_urdf`` -- the box fallback of optimizer.py ``_getLinkCollisionGeometry`` from the reference's own
  ``link_cuboid_hulls``, or from the no-mesh branches of ``getBoundingBox`` / ``getLinkGeometry``.
* ``world_boxes_from_urdf`` -- the static boxes of a world URDF (``getLinkWorldTransforms`` composed with the visual origin).
* ``collision_pairs`` -- excitation/trajectoryOptimizer.py ``_buildCollisionPairs``: ``ignoreLinksForCollision``,
  ``ignoreLinkPairsForCollision``, ``ignoreCollisionBetweenGroups``, neighbours skipped, ``collisionMaxKinematicDistance``, world-world pairs
  skipped, in the reference's pair order.
* ``read_stl``, ``Hull``, ``hull_from_box``, ``hulls_from_urdf``, ``world_hulls_from_urdf`` -- optimizer.py ``_getLinkCollisionGeometry``
  for ``collisionMode: "convex"``: the convex hull of the link's collision (else visual) mesh times the URDF scale, a box for links
  without a mesh and for all world links.
* ``Mesh``, ``meshes_from_urdf`` -- ``_getLinkCollisionGeometry`` for ``link_mode == "full"``: the triangles of the same mesh, for the links of
  ``fullMeshLinks`` (concave shapes such as the cage around WALK-MAN's torso, whose hull is more than 80 % empty space) or, in
  ``collisionMode: "full"``, for every link that has a mesh.  A mesh distance is the minimum over the triangles, exactly 0.0 where the two
  touch or intersect and never negative; a geometry wholly inside a closed mesh has a positive distance, as with FCL's BVH.
* ``collision_set`` -- all of it in the form ``Engine.set_capsules`` / ``Engine.set_boxes`` / ``Engine.set_hulls`` and the ``collision``
  argument of ``excitation.candidate_objectives`` take.

The distances themselves are computed on the device (``Engine.candidate_capsule_distances``, csrc/fbr_capsule.h;
``Engine.candidate_box_distances``, csrc/fbr_box.h; ``Engine.candidate_hull_distances``, csrc/fbr_hull.h and, for pairs with a mesh, csrc/fbr_mesh.h; their
gradients: ``Engine.mesh_distance_gradients``, csrc/fbr_mesh_grad.h, behind ``mesh_gradient=True`` of ``flobaroid_amd.excitation``).  Hulls of
``FBR_MAX_HULL_VERTICES`` + 1 to ``FBR_MAX_LARGE_HULL_VERTICES`` vertices (KUKA LWR4: the hulls of its visual meshes) are served for
distances only: ``hulls_from_urdf(..., max_vertices=FBR_MAX_LARGE_HULL_VERTICES)`` and ``Engine.set_hulls(..., large=True)``,
csrc/fbr_hull_large.h.  Meshes of ``FBR_MAX_MESH_TRIANGLES`` + 1 to ``FBR_MAX_LARGE_MESH_TRIANGLES`` triangles, mesh pairs above
``FBR_MAX_MESH_PAIR_WORK`` and meshes on such hulls (KUKA LWR4 in ``collisionMode: "full"``) are served for distances only, through a
bounding-sphere tree per mesh: ``meshes_from_urdf(..., max_triangles=FBR_MAX_LARGE_MESH_TRIANGLES)``, ``collision_set(...,
large_meshes=True)`` and ``Engine.set_large_hull_meshes``, csrc/fbr_mesh_bvh.h.  Not covered: gradients of meshes attached that way;
meshes whose hull has more than ``FBR_MAX_LARGE_HULL_VERTICES`` vertices or that have more than ``FBR_MAX_LARGE_MESH_TRIANGLES``
triangles (no simplification); formats other than STL; parity with FCL's own numbers.
"""
from __future__ import annotations

import os
import xml.etree.ElementTree as ET
from dataclasses import dataclass, field

import numpy as np

FBR_MAX_HULL_VERTICES = 128  # include/fbr.h: Engine.set_hulls
FBR_MAX_LARGE_HULL_VERTICES = 1024  # include/fbr.h: Engine.set_hulls(..., large=True), distances only
FBR_MAX_MESH_TRIANGLES = 256  # include/fbr.h
FBR_MAX_LARGE_MESH_TRIANGLES = 8192  # include/fbr.h: Engine.set_large_hull_meshes, collision_set(..., large_meshes=True), distances only
FBR_MAX_MESH_PAIR_WORK = 32768  # include/fbr.h: triangles x triangles of one pair
_COPLANAR = 1e-10            # x the hull's diameter: neighbouring triangles this flat against each other are one face


@dataclass
class Capsule:
    """A segment ``p0_local`` -- ``p1_local`` in the frame of link ``link_name`` plus a radius (p0 == p1: a sphere)."""

    link_name: str
    p0_local: np.ndarray
    p1_local: np.ndarray
    radius: float


@dataclass
class Box:
    """An oriented box.  ``link_name`` a robot link: the box has the link's axes and sits ``center`` off the link origin (``rot`` is None);
    ``link_name`` None: a world box, ``center`` and ``rot`` (3, 3, columns = box axes) in the world, ``name`` the world link it came from."""

    link_name: str | None
    half: np.ndarray
    center: np.ndarray
    rot: np.ndarray | None = None
    name: str | None = None


@dataclass
class Hull:
    """A convex polytope.  ``vertices`` (V, 3) in the axes of link ``link_name``, relative to a point ``offset`` off the link origin
    (``rot`` is None); ``link_name`` None: a world hull, ``offset`` and ``rot`` (3, 3) in the world, ``name`` the world link it came from.
    The points given are reduced to the vertices of their convex hull (Qhull), and the tables the device needs are derived:
    ``planes`` (F, 4), unit outward normal | offset (n . x <= o inside), one row per MERGED face -- Qhull's triangles are joined while the
    opposite vertex of a neighbour lies within 1e-10 x the diameter of the plane --, and ``edges`` (E, 4) int32, the two end vertices and
    the two merged faces that meet there (edges between triangles of one face are dropped).  ``bounds`` (2, 3): the axis-aligned
    bounding box of the points, when the hull came from a mesh.  Fewer than 4 points, or a flat set, raise ValueError."""

    link_name: str | None
    vertices: np.ndarray
    offset: np.ndarray
    rot: np.ndarray | None = None
    name: str | None = None
    bounds: np.ndarray | None = None
    planes: np.ndarray = field(init=False, repr=False)
    edges: np.ndarray = field(init=False, repr=False)

    def __post_init__(self):
        from scipy.spatial import ConvexHull, QhullError

        pts = np.asarray(self.vertices, dtype=np.float64).reshape(-1, 3)
        self.offset = np.asarray(self.offset, dtype=np.float64).reshape(3)
        who = self.link_name or self.name or "hull"
        if len(pts) < 4 or not np.isfinite(pts).all():
            raise ValueError(f"{who}: a hull needs 4 finite points at least")
        try:
            qh = ConvexHull(pts)
        except (QhullError, ValueError) as e:
            raise ValueError(f"{who}: no convex hull of these points (flat?): {str(e).splitlines()[0]}") from None
        diam = float(np.linalg.norm(pts[qh.vertices][:, None] - pts[qh.vertices][None], axis=2).max())
        tri, eq, nb = qh.simplices, qh.equations, qh.neighbors
        group = list(range(len(tri)))

        def find(i):
            while group[i] != i:
                group[i] = group[group[i]]
                i = group[i]
            return i

        for i in range(len(tri)):
            for k in range(3):  # (neighbour k lies opposite vertex k: its own vertex that is not shared is the one to test)
                j = int(nb[i, k])
                far = [x for x in tri[j] if x not in tri[i]]
                if j > i and far and abs(eq[i, :3] @ pts[far[0]] + eq[i, 3]) <= _COPLANAR * diam and eq[i, :3] @ eq[j, :3] > 0:
                    group[find(j)] = find(i)
        roots = sorted({find(i) for i in range(len(tri))})
        face_of = {r: f for f, r in enumerate(roots)}
        area = np.linalg.norm(np.cross(pts[tri[:, 1]] - pts[tri[:, 0]], pts[tri[:, 2]] - pts[tri[:, 0]]), axis=1)
        planes = np.zeros((len(roots), 4))
        for r in roots:  # the plane of a merged face: that of its largest triangle
            members = [i for i in range(len(tri)) if find(i) == r]
            i = members[int(np.argmax(area[members]))]
            nrm = eq[i, :3] / np.linalg.norm(eq[i, :3])
            planes[face_of[r]] = [*nrm, -eq[i, 3] / np.linalg.norm(eq[i, :3])]
        edges = []
        for i in range(len(tri)):
            for k in range(3):
                j = int(nb[i, k])
                if j > i and find(i) != find(j):
                    a, b = (int(x) for x in tri[i] if x != tri[i][k])
                    edges.append((a, b, face_of[find(i)], face_of[find(j)]))
        used = sorted({v for e in edges for v in e[:2]})  # (a point inside a merged face is no vertex)
        renum = {v: i for i, v in enumerate(used)}
        self.vertices = np.ascontiguousarray(pts[used])
        self.planes = planes
        self.edges = np.array([(renum[a], renum[b], f, g) for a, b, f, g in edges], dtype=np.int32).reshape(-1, 4)
        if len(used) < 4 or len(planes) < 4:
            raise ValueError(f"{who}: the hull of these points is flat")

    @property
    def diameter(self) -> float:
        return float(np.linalg.norm(self.vertices[:, None] - self.vertices[None], axis=2).max())


@dataclass
class Mesh:
    """A triangle mesh of link ``link_name``: ``triangles`` (T, 3, 3) in the axes of the link, relative to ``offset`` -- the axes and the
    origin of ``hull``, the ``Hull`` of the mesh's vertices, which stays in the hull set (it bounds the mesh).  Zero-area triangles are kept."""

    link_name: str
    triangles: np.ndarray
    offset: np.ndarray
    hull: Hull = field(init=False, repr=False)

    def __post_init__(self):
        self.triangles = np.ascontiguousarray(np.asarray(self.triangles, dtype=np.float64).reshape(-1, 3, 3))
        self.offset = np.asarray(self.offset, dtype=np.float64).reshape(3)
        if len(self.triangles) == 0 or not np.isfinite(self.triangles).all():
            raise ValueError(f"{self.link_name}: a mesh needs one finite triangle at least")
        pts = self.triangles.reshape(-1, 3)
        self.hull = Hull(self.link_name, pts, self.offset, bounds=np.array([pts.min(axis=0), pts.max(axis=0)]))


def read_stl(path) -> np.ndarray:
    """The triangles (ntri, 3, 3) float64 of a binary or an ASCII STL file.  Any other mesh format raises ValueError naming the file."""
    with open(path, "rb") as fh:
        raw = fh.read()
    if len(raw) >= 84:
        ntri = int(np.frombuffer(raw, dtype="<u4", count=1, offset=80)[0])
        if len(raw) == 84 + 50 * ntri:  # 80 bytes of header, the count, 50 bytes a triangle: normal, three vertices, two bytes
            rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=ntri, offset=84)
            return rec["v"].astype(np.float64)
    if raw.lstrip()[:5].lower() == b"solid":
        try:
            v = [[float(x) for x in ln.split()[1:4]] for ln in raw.decode("ascii", "replace").splitlines() if ln.strip().lower().startswith("vertex")]
        except ValueError:
            v = []
        if v and len(v) % 3 == 0:
            return np.array(v, dtype=np.float64).reshape(-1, 3, 3)
    raise ValueError(f"{path}: neither a binary nor an ASCII STL file (other mesh formats are not read)")


def hull_from_box(box: Box) -> Hull:
    """The 8 vertices, 6 faces and 12 edges of ``box``; ``offset`` is the box centre."""
    corners = np.array([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]) * np.asarray(box.half, dtype=np.float64)
    return Hull(box.link_name, corners, box.center, None if box.rot is None else np.asarray(box.rot, dtype=np.float64), box.name)


def _mesh_file(urdf, link, mesh_base_dir):
    """(path or None, scale (3,)) of the link's collision mesh, else its visual mesh -- ``_getMeshPathFromTag`` without ROS: a
    ``package://`` / ``model://`` name is cut from ``mesh_base_dir`` on and taken relative to the URDF's directory."""
    for tag in ("collision/geometry/mesh", "visual/geometry/mesh"):
        m = link.find(tag)
        if m is None:
            continue
        path = m.attrib["filename"]
        if path.startswith("package") or path.startswith("model"):
            parts = path.split("/")
            if mesh_base_dir not in parts:
                continue
            path = os.path.join(os.path.dirname(os.path.abspath(urdf)), *parts[parts.index(mesh_base_dir):])
        if os.path.exists(path):
            return path, np.array([float(v) for v in m.attrib.get("scale", "1 1 1").split()])
    return None, None


def hulls_from_urdf(urdf, link_names, mesh_base_dir: str = "meshes", x_std=None, cube_size=None, scale: float = 1.0,
                    max_vertices: int = FBR_MAX_HULL_VERTICES):
    """``(hulls, box_links)``: optimizer.py ``_getLinkCollisionGeometry`` for ``link_mode == "convex"``.  A link whose collision mesh, else
    visual mesh, is an STL file that exists gets the convex hull of the mesh vertices times the URDF ``scale`` (signs included); its
    ``offset`` is the position ``getBoundingBox`` returns -- ``visual/origin`` xyz, else ``collision/origin`` xyz -- and the rotation of
    that origin is NOT applied to the vertices, as in the reference.  ``Hull.bounds`` is ``mesh.bounding_box.bounds * scale``.  Every
    other link (no mesh, or the file is missing) is listed in ``box_links`` and gets the box of ``boxes_from_urdf`` (``x_std``,
    ``cube_size``, ``scale`` = ``scaleCollisionHull`` as there) through ``hull_from_box``; a link without any geometry gets nothing.  A
    hull with more than ``max_vertices`` vertices raises ValueError naming the link and its count: no simplification is attempted.  A
    robot with visual meshes only (KUKA LWR4) passes ``max_vertices=FBR_MAX_LARGE_HULL_VERTICES``."""
    tree = ET.parse(urdf)
    wanted = list(link_names)
    boxes, _ = boxes_from_urdf(urdf, wanted, x_std=x_std, cube_size=cube_size, scale=scale)
    found, box_links = {}, []
    for link in tree.findall("link"):
        name = link.attrib["name"]
        if name not in wanted:
            continue
        path, mscale = _mesh_file(urdf, link, mesh_base_dir)
        if path is None:
            box_links.append(name)
            if name in boxes:
                found[name] = hull_from_box(boxes[name])
            continue
        pts = read_stl(path).reshape(-1, 3) * mscale
        origin = link.find("visual/origin")
        if origin is None:
            origin = link.find("collision/origin")
        h = Hull(name, pts, _origin(origin)[0], bounds=np.array([pts.min(axis=0), pts.max(axis=0)]))
        if len(h.vertices) > max_vertices:
            raise ValueError(f"link {name}: the hull of {os.path.basename(path)} has {len(h.vertices)} vertices, more than {max_vertices}")
        found[name] = h
    return {n: found[n] for n in wanted if n in found}, box_links


def meshes_from_urdf(urdf, link_names, mesh_base_dir: str = "meshes", max_triangles: int = FBR_MAX_MESH_TRIANGLES) -> dict:
    """{link: Mesh}: optimizer.py ``_getLinkCollisionGeometry`` for ``link_mode == "full"``, for the links of ``link_names`` only (no other
    link's file is read).  The collision mesh, else the visual mesh, times the URDF ``scale``; the rotation of the origin is NOT applied and
    the offset (``visual/origin`` xyz, else ``collision/origin`` xyz) is added in world axes -- the reference's behaviour, exactly as
    ``hulls_from_urdf`` documents it, so that ``Mesh.hull`` is the hull ``hulls_from_urdf`` gives the link.  Triangle winding is irrelevant to
    a distance (a negative scale is applied as it is).  A requested link that is not in the URDF or has no STL file that exists raises
    ValueError naming it; more than ``max_triangles`` triangles: ValueError with link, file and count (no simplification is attempted)."""
    tree = ET.parse(urdf)
    wanted = list(link_names)
    found = {}
    for link in tree.findall("link"):
        name = link.attrib["name"]
        if name not in wanted:
            continue
        path, mscale = _mesh_file(urdf, link, mesh_base_dir)
        if path is None:
            raise ValueError(f"link {name}: no STL file for its collision or visual mesh (a triangle mesh was asked for)")
        tri = read_stl(path) * mscale
        if len(tri) > max_triangles:
            raise ValueError(f"link {name}: {os.path.basename(path)} has {len(tri)} triangles, more than {max_triangles}")
        origin = link.find("visual/origin")
        if origin is None:
            origin = link.find("collision/origin")
        found[name] = Mesh(name, tri, _origin(origin)[0])
    missing = [n for n in wanted if n not in found]
    if missing:
        raise ValueError(f"link(s) {missing}: not in {os.path.basename(urdf)}")
    return {n: found[n] for n in wanted}


def world_hulls_from_urdf(world_urdf, placement: str = "reference", cube_size=None) -> dict:
    """{world link: Hull}: world links are always boxes in the reference (it looks their mesh up in the ROBOT's URDF) --
    ``world_boxes_from_urdf`` in either placement, through ``hull_from_box``."""
    return {n: hull_from_box(b) for n, b in world_boxes_from_urdf(world_urdf, placement, cube_size).items()}


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


def collision_pairs(topology, capsules, config: dict, world_links=(), boxes=None) -> list:
    """Link pairs ``(l0, l1)`` (names, l0 before l1 in ``topology.link_names + world_links``) the optimiser checks, in its order.  Skipped:
    robot links without geometry (neither in ``capsules`` nor in ``boxes``) or in ``ignoreLinksForCollision``; pairs in
    ``ignoreLinkPairsForCollision`` (either order) or across two groups of ``ignoreCollisionBetweenGroups``; neighbours
    (``link_neighbors``); with ``collisionMaxKinematicDistance`` > 0, pairs further apart than that many steps of the neighbour graph --
    which, as in the reference, drops EVERY pair with a world link (a world link is not in the graph: distance 999); world-world pairs."""
    names = list(topology.link_names)
    nrobot = len(names)
    all_links = names + [w for w in world_links]
    have = set(capsules) | set(boxes or {})
    ignore_links = set(config.get("ignoreLinksForCollision", [])) | {n for n in names if n not in have}
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
    for i, l0 in enumerate(all_links):
        for j in range(i + 1, len(all_links)):
            l1 = all_links[j]
            if i >= nrobot and j >= nrobot:
                continue
            if l0 in ignore_links or l1 in ignore_links:
                continue
            if (l0, l1) in ignore_pairs or (l0, l1) in group_ignore:
                continue
            if i < nrobot and j < nrobot and (l0 in nbs[l1] or l1 in nbs[l0]):
                continue
            if max_dist > 0 and kin_distance(l0, l1) > max_dist:
                continue
            pairs.append((l0, l1))
    return pairs


def _euler_to_matrix(rpy):
    return _origin(type("O", (), {"attrib": {"rpy": " ".join(repr(float(v)) for v in rpy)}})())[1]


def _matrix_to_euler(R):
    """the reference's rotationMatrixToEulerAngles (its singular branch included)"""
    sy = np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0])
    if sy >= 1e-6:
        return np.array([np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], sy), np.arctan2(R[1, 0], R[0, 0])])
    return np.array([np.arctan2(-R[1, 2], R[1, 1]), np.arctan2(-R[2, 0], sy), 0.0])


def _link_geometry(link):
    """getLinkGeometry for one <link>: (size (3,), position, rpy-matrix) of the first box / cylinder / sphere -- visual geometry before
    collision geometry, the origin always the VISUAL one -- or None; and whether the link names a mesh."""
    vo = link.find("visual/origin")
    pos, rot = _origin(vo)
    has_mesh = link.find("visual/geometry/mesh") is not None or link.find("collision/geometry/mesh") is not None
    for prefix in ("visual/geometry", "collision/geometry"):
        m = link.find(prefix + "/box")
        if m is not None:
            return np.array([float(v) for v in m.attrib["size"].split()]), pos, rot, has_mesh
        m = link.find(prefix + "/cylinder")
        if m is not None:
            r, length = float(m.attrib["radius"]), float(m.attrib["length"])
            return np.array([2 * r, 2 * r, length]), pos, rot, has_mesh
        m = link.find(prefix + "/sphere")
        if m is not None:
            r = float(m.attrib["radius"])
            return np.array([2 * r, 2 * r, 2 * r]), pos, rot, has_mesh
    return None, pos, rot, has_mesh


def boxes_from_hulls(link_cuboid_hulls: dict, robot_links, scale: float = 1.0):
    """``(boxes, world_boxes)`` from the reference's ``link_cuboid_hulls`` ({link: [box (2, 3) min | max, pos, rot]}, what a caller with
    trimesh has): the arithmetic of optimizer.py:629-633.  A robot link's box is scaled by ``scale`` (``scaleCollisionHull``), its centre
    ``0.5 (b0 + b1) scale + pos`` is an offset from the link origin; every other entry is a world box, unscaled, placed as the reference
    places it: at ``pos + (0.5 (b0 + b1) + pos)`` with the rotation of ``rot`` (Euler angles or a matrix)."""
    robot = set(robot_links)
    boxes, world = {}, {}
    for name, (box, pos, rot) in link_cuboid_hulls.items():
        b = np.asarray(box, dtype=np.float64) * (scale if name in robot else 1.0)
        p = np.asarray(pos, dtype=np.float64)
        center = 0.5 * (b[0] + b[1]) + p
        if name in robot:
            boxes[name] = Box(name, 0.5 * (b[1] - b[0]), center)
        else:
            R = _euler_to_matrix(rot) if np.ndim(rot) == 1 else np.asarray(rot, dtype=np.float64)
            world[name] = Box(None, 0.5 * (b[1] - b[0]), p + center, R, name)
    return boxes, world


def boxes_from_urdf(urdf, link_names, x_std=None, cube_size=None, scale: float = 1.0):
    """``(boxes, mesh_links)``: the boxes ``boxes_from_hulls`` gives for the hulls the reference builds WITHOUT a mesh: a link with
    ``box`` / ``cylinder`` / ``sphere`` geometry gets that primitive's bounding box at the visual origin's position (its rotation is not
    used, as in the reference).  A link that names a mesh is listed in ``mesh_links`` (there is no mesh code here); with ``cube_size`` and
    ``x_std`` it gets what the reference falls back to when the mesh file is missing: the cube of that edge around the a-priori centre of
    mass.  Links without any geometry get no box (the reference skips them: ``hasVisualGeometry``)."""
    tree = ET.parse(urdf)
    wanted = list(link_names)
    hulls, mesh_links = {}, []
    for link in tree.findall("link"):
        name = link.attrib["name"]
        if name not in wanted:
            continue
        size, pos, _, has_mesh = _link_geometry(link)
        if has_mesh:
            mesh_links.append(name)
            if cube_size is not None and x_std is not None:
                i = wanted.index(name)
                m = float(x_std[10 * i])
                com = np.asarray(x_std[10 * i + 1:10 * i + 4], dtype=np.float64) / m if m != 0 else np.zeros(3)
                hulls[name] = [np.array([com - 0.5 * cube_size, com + 0.5 * cube_size]), np.zeros(3), np.eye(3)]
        elif size is not None and np.any(size != 0):
            hulls[name] = [np.array([-0.5 * size, 0.5 * size]), pos, np.eye(3)]
    return boxes_from_hulls(hulls, wanted, scale)[0], mesh_links


def world_boxes_from_urdf(world_urdf, placement: str = "reference", cube_size=None) -> dict:
    """{world link: Box} of a static world URDF, in document order -- every link with child elements (``getLinkNames``), its primitive's
    bounding box (``cube_size``: the cube a link without one gets; None: such a link is an error), the joint chain's transform
    (``getLinkWorldTransforms``: fixed joints, from the root) composed with the visual origin as optimizer.py:507-525 does:
    ``pos = link_pos + link_rot visual_pos``, ``rot = link_rot visual_rot``.

    ``placement="reference"`` reproduces where the reference's collision loop puts the box: ``_getLinkTransform`` returns ``pos`` and
    ``_getLinkCollisionGeometry`` returns the offset ``mid + pos``, and the loop adds the two -- the box lands at ``2 pos + mid``, with the
    rotation taken through Euler angles and back.  ``"geometric"`` places it where the URDF says: ``pos + rot mid``."""
    if placement not in ("reference", "geometric"):
        raise ValueError("placement: 'reference' or 'geometric'")
    root = ET.parse(world_urdf).getroot()
    parent = {}
    for joint in root.findall("joint"):
        p, c = joint.find("parent"), joint.find("child")
        if p is None or c is None:
            continue
        parent[c.attrib["link"]] = (p.attrib["link"],) + _origin(joint.find("origin"))
    done = {}

    def transform(name):
        if name not in done:
            if name not in parent:
                done[name] = (np.zeros(3), np.eye(3))
            else:
                pn, xyz, R = parent[name]
                pp, pR = transform(pn)
                done[name] = (pp + pR @ xyz, pR @ R)
        return done[name]

    out = {}
    for link in root.findall("link"):
        if len(list(link)) == 0:  # (a frame only)
            continue
        name = link.attrib["name"]
        size, vpos, vrot, _ = _link_geometry(link)
        if size is not None and np.any(size != 0):
            b = np.array([-0.5 * size, 0.5 * size])
        elif cube_size is not None:
            b, vpos, vrot = np.array([np.full(3, -0.5 * cube_size), np.full(3, 0.5 * cube_size)]), np.zeros(3), np.eye(3)
        else:
            raise ValueError(f"world link {name} has no box, cylinder or sphere geometry (cube_size: the cube the reference gives it)")
        lpos, lrot = transform(name)
        pos, R = lpos + lrot @ vpos, lrot @ vrot
        mid = 0.5 * (b[0] + b[1])
        if placement == "reference":
            out[name] = Box(None, 0.5 * (b[1] - b[0]), pos + (mid + pos), _euler_to_matrix(_matrix_to_euler(R)), name)
        else:
            out[name] = Box(None, 0.5 * (b[1] - b[0]), pos + R @ mid, R, name)
    return out


def collision_set(topology, capsules, config: dict, margins=None, boxes=None, world_boxes=None, hulls=None, world_hulls=None, meshes=None,
                  large_meshes: bool = False) -> dict:
    """What ``Engine.set_capsules`` / ``Engine.set_boxes`` and the ``collision`` argument of ``excitation.candidate_objectives`` take.

    Without ``boxes`` and ``world_boxes``: ``capsules`` (a list, one per link that has one, in link order), ``pairs`` ((P, 2) indices into
    that list, from ``collision_pairs``), ``pair_names`` and ``margins`` ((P,), default 0: the reference's ``_collision_pair_margins`` are
    zero for pairs of robot links).

    With ``boxes`` ({robot link: Box}) and / or ``world_boxes`` ({world link: Box}, their order is the order of the world links):
    ``pair_names`` is the reference's list over robot and world links, and every pair is served as the reference serves it -- in
    ``collisionMode: "capsule"`` by the capsule routine when both links have a capsule, by the box routine otherwise; in ``"box"`` always
    by the box routine.  ``pairs`` then holds the capsule pairs only, and there are in addition ``boxes`` (a list: robot boxes in link
    order, then the world boxes), ``box_pairs`` ((Pb, 2) into that list), ``columns`` ((P, 2): per pair of ``pair_names`` the set -- 0
    capsules, 1 boxes -- and the column of that set's result that serves it) and ``margins`` default to ``worldCollisionMargin`` on pairs
    with a world link, 0 elsewhere.  A pair that needs a box for a link that has none is an error.

    With ``hulls`` ({robot link: Hull}, and ``world_hulls`` {world link: Hull}): ``collisionMode: "convex"``.  ``pair_names`` is the
    reference's list with the hull links in the role the box links play in box mode, every pair is served by the hull routine
    (``columns[:, 0] == 2``), and there are ``hulls`` (a list: robot hulls in link order, then the world hulls), ``hull_pairs`` ((P, 2)
    into that list, sorted so that a pair's first hull changes rarely; ``columns[:, 1]`` says where a pair of ``pair_names`` went) and
    ``offset_in_link_axes`` (False: the reference's placement).  Margins default as for boxes.  Without ``meshes``, ``fullMeshLinks`` and
    ``collisionMode: "full"`` are refused.

    With ``meshes`` ({robot link: Mesh}, from ``meshes_from_urdf``) beside ``hulls``: ``fullMeshLinks`` is accepted -- every link named
    there must be in ``meshes`` and is served as its triangle mesh, every other link as its hull -- and so is ``collisionMode: "full"``, in
    which EVERY robot link in ``meshes`` is a mesh and the others are their hull or box, as in the reference.  A meshed link's hull is
    ``Mesh.hull`` (it replaces the entry of ``hulls``, if any).  The dict gains ``meshes`` ({hull index: triangles (T, 3, 3)}: what
    ``Engine.set_hull_meshes`` takes); pair order, ``columns`` and margins are as in convex mode.  A mesh above ``FBR_MAX_MESH_TRIANGLES``
    or a pair above ``FBR_MAX_MESH_PAIR_WORK`` triangle pairs raises ValueError naming the links and the counts.

    ``large_meshes=True`` (with ``meshes``): the meshes go to ``Engine.set_large_hull_meshes`` -- the cap of a mesh is
    ``FBR_MAX_LARGE_MESH_TRIANGLES``, a pair has no cap, the hulls may have up to ``FBR_MAX_LARGE_HULL_VERTICES`` vertices, and the dict
    carries ``"large_meshes": True`` (KUKA LWR4 in ``collisionMode: "full"``).  Distances only: the gradient entry points refuse the set."""
    if hulls is not None:
        mode = config.get("collisionMode", "convex")
        full = list(config.get("fullMeshLinks", []) or [])
        if (full or mode == "full") and meshes is None:
            raise ValueError(f"collisionMode 'full' and fullMeshLinks {list(config.get('fullMeshLinks', []))} need triangle meshes: not covered")
        if mode not in ("convex", "full"):
            raise ValueError("hulls serve collisionMode 'convex' (boxes= / world_boxes= serve 'capsule' and 'box')")
        hulls, world_hulls = dict(hulls), dict(world_hulls or {})
        meshed = {}
        if meshes is not None:
            lacking = [n for n in full if n not in meshes]
            if lacking:
                raise ValueError(f"fullMeshLinks {lacking}: no mesh given for them (meshes=)")
            meshed = {n: meshes[n] for n in (meshes if mode == "full" else full) if n in topology.link_names}
            for n, mm in meshed.items():
                cap = FBR_MAX_LARGE_MESH_TRIANGLES if large_meshes else FBR_MAX_MESH_TRIANGLES
                if len(mm.triangles) > cap:
                    raise ValueError(f"link {n}: {len(mm.triangles)} triangles, more than {cap}")
                hulls[n] = mm.hull
        clash = set(world_hulls) & set(topology.link_names)
        if clash:
            raise ValueError(f"link(s) {sorted(clash)} declared in the model and in the world")
        pair_names = collision_pairs(topology, {}, config, world_links=list(world_hulls), boxes=hulls)
        hnames = [n for n in topology.link_names if n in hulls] + list(world_hulls)
        hpos = {n: i for i, n in enumerate(hnames)}
        raw = [(hpos[a], hpos[b]) for a, b in pair_names]
        order = sorted(range(len(raw)), key=lambda k: (raw[k][0], k))
        columns = np.zeros((len(raw), 2), dtype=np.int64)
        columns[:, 0] = 2
        columns[order, 1] = np.arange(len(raw))
        if margins is None:
            wm = float(config.get("worldCollisionMargin", 0.0))
            m = np.array([wm if (a in world_hulls or b in world_hulls) else 0.0 for a, b in pair_names])
        else:
            m = np.asarray(margins, dtype=np.float64).reshape(len(pair_names))
        out = {"capsules": [], "pairs": np.zeros((0, 2), dtype=np.int32), "pair_names": pair_names, "margins": m,
               "hulls": [hulls[n] if n in hulls else world_hulls[n] for n in hnames],
               "hull_pairs": np.array([raw[k] for k in order], dtype=np.int32).reshape(-1, 2), "columns": columns, "offset_in_link_axes": False}
        if meshes is not None:
            for a, b in pair_names:
                if large_meshes:
                    break  # (the trees bound the work of a pair)
                if a in meshed and b in meshed and len(meshed[a].triangles) * len(meshed[b].triangles) > FBR_MAX_MESH_PAIR_WORK:
                    raise ValueError(f"pair ({a}, {b}): {len(meshed[a].triangles)} x {len(meshed[b].triangles)} triangle pairs, more than "
                                     f"{FBR_MAX_MESH_PAIR_WORK}")
            out["meshes"] = {hpos[n]: meshed[n].triangles for n in hnames if n in meshed}
            if large_meshes:
                out["large_meshes"] = True
        return out
    names = [n for n in topology.link_names if n in capsules]
    pos = {n: i for i, n in enumerate(names)}
    if boxes is None and world_boxes is None:
        pair_names = collision_pairs(topology, capsules, config)
        pairs = np.array([(pos[a], pos[b]) for a, b in pair_names], dtype=np.int32).reshape(-1, 2)
        m = np.zeros(len(pair_names)) if margins is None else np.asarray(margins, dtype=np.float64).reshape(len(pair_names))
        return {"capsules": [capsules[n] for n in names], "pairs": pairs, "pair_names": pair_names, "margins": m}
    mode = config.get("collisionMode", "capsule")
    if mode not in ("capsule", "box"):
        raise ValueError("collision sets cover collisionMode 'capsule' and 'box' (no mesh code); 'convex' needs hulls=")
    boxes, world_boxes = dict(boxes or {}), dict(world_boxes or {})
    clash = set(world_boxes) & set(topology.link_names)
    if clash:
        raise ValueError(f"link(s) {sorted(clash)} declared in the model and in the world")
    caps = capsules if mode == "capsule" else {}
    pair_names = collision_pairs(topology, capsules, config, world_links=list(world_boxes), boxes=boxes)
    bnames = [n for n in topology.link_names if n in boxes] + list(world_boxes)
    bpos = {n: i for i, n in enumerate(bnames)}
    cap_pairs, box_pairs, columns = [], [], []
    for a, b in pair_names:
        if a in caps and b in caps:
            columns.append((0, len(cap_pairs)))
            cap_pairs.append((pos[a], pos[b]))
        else:
            for n in (a, b):
                if n not in bpos:
                    raise ValueError(f"pair ({a}, {b}) goes to the box routine, but {n} has no box")
            columns.append((1, len(box_pairs)))
            box_pairs.append((bpos[a], bpos[b]))
    if margins is None:
        wm = float(config.get("worldCollisionMargin", 0.0))
        m = np.array([wm if (a in world_boxes or b in world_boxes) else 0.0 for a, b in pair_names])
    else:
        m = np.asarray(margins, dtype=np.float64).reshape(len(pair_names))
    return {"capsules": [capsules[n] for n in names] if mode == "capsule" else [],
            "pairs": np.array(cap_pairs, dtype=np.int32).reshape(-1, 2), "pair_names": pair_names, "margins": m,
            "boxes": [boxes[n] if n in boxes else world_boxes[n] for n in bnames], "box_pairs": np.array(box_pairs, dtype=np.int32).reshape(-1, 2),
            "columns": np.array(columns, dtype=np.int64).reshape(-1, 2)}
