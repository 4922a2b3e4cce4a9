"""Shapes and a robot for the hull tests (tests/test_hulls.py, tests/test_gpu_hulls.py): polytopes at the vertex cap of the device
(FBR_MAX_HULL_VERTICES 128), round ones, an apex where every side face meets, very small and very large ones, and a gantry of two
prismatic joints whose poses are exact in fp64, so that a chosen joint value puts two hulls at a known gap.

Counts (vertices / merged faces / edges): prism(64) 128 / 66 / 192, fibonacci_sphere(128) 128 / 252 / 378, cone(127) 128 / 128 / 254,
prism(6) 12 / 8 / 18, a box 8 / 6 / 12, wedge 6 / 5 / 9, a tetrahedron 4 / 4 / 6 (tests/test_hulls.py asserts them)."""
import numpy as np

KINDS = ("prism128", "sphere128", "cone128", "box", "hexprism", "tiny", "slab", "tetra")
COUNTS = {"prism128": (128, 66, 192), "sphere128": (128, 252, 378), "cone128": (128, 128, 254), "box": (8, 6, 12), "hexprism": (12, 8, 18),
          "tiny": (20, 36, 54), "slab": (8, 6, 12), "tetra": (4, 4, 6)}


def prism(n, r, h):
    """(2 n, 3): an n-gon of circumradius r in the planes z = -h / 2 and z = h / 2; vertex k at the angle 2 pi k / n"""
    t = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([r * np.cos(t), r * np.sin(t)], axis=1)
    return np.concatenate([np.concatenate([ring, np.full((n, 1), z)], axis=1) for z in (-0.5 * h, 0.5 * h)])


def fibonacci_sphere(n, r):
    """(n, 3): n points on the sphere of radius r about the origin, on the golden-angle spiral (every one is a vertex of their hull)"""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = np.pi * (3.0 - np.sqrt(5.0)) * k
    s = np.sqrt(1.0 - z * z)
    return r * np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


def cone(n, r, h):
    """(n + 1, 3): an n-gon of circumradius r in the plane z = 0 and the apex (0, 0, h), the last row: n side faces meet there"""
    t = 2.0 * np.pi * np.arange(n) / n
    return np.concatenate([np.stack([r * np.cos(t), r * np.sin(t), np.zeros(n)], axis=1), [[0.0, 0.0, h]]])


def wedge(a, b, c, along="y"):
    """(6, 3): a roof over the rectangle |x| <= a, |y| <= b in the plane z = 0 whose ridge, at the height c, runs along y from -b to b
    (``along`` "x": the same turned by a quarter about z).  Dyadic a, b, c give exact coordinates."""
    v = np.array([[-a, -b, 0.0], [a, -b, 0.0], [-a, b, 0.0], [a, b, 0.0], [0.0, -b, c], [0.0, b, c]])
    return v if along == "y" else v[:, [1, 0, 2]] * np.array([-1.0, 1.0, 1.0])


def tetra(rng, size):
    """(4, 3): four normal points of scale ``size``: the smallest hull the device takes"""
    return rng.standard_normal((4, 3)) * size


def box(half):
    return np.array([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]) * np.asarray(half, dtype=np.float64)


def zoo(rng, link, kind):
    """a flobaroid_amd.collision.Hull of one of KINDS on ``link`` (a name; None: a world hull with a random rotation), sizes a few
    decimetres but for "tiny" (a 20-point sphere of 1 mm radius) and "slab" (10 m x 10 m x 1 m), the offset a few centimetres"""
    from flobaroid_amd.collision import Hull

    s = rng.uniform(0.8, 1.25)
    pts = {"prism128": lambda: prism(64, 0.25 * s, 0.3 * s), "sphere128": lambda: fibonacci_sphere(128, 0.25 * s),
           "cone128": lambda: cone(127, 0.25 * s, 0.4 * s), "box": lambda: box(rng.uniform(0.1, 0.3, 3)), "hexprism": lambda: prism(6, 0.2 * s, 0.35 * s),
           "tiny": lambda: fibonacci_sphere(20, 1e-3), "slab": lambda: box([5.0, 5.0, 0.5]), "tetra": lambda: tetra(rng, 0.15 * s)}[kind]()
    rot = None
    if link is None:
        from scipy.spatial.transform import Rotation

        rot = Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix()
    return Hull(link, pts, rng.uniform(-0.03, 0.03, 3), rot, None if link is not None else "world_" + kind)


TURNS = {"upright": np.eye(3), "apex_down": np.diag([1.0, -1.0, -1.0]),                                   # pi about x
         "on_side": np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]),                         # pi / 2 about x
         "quarter": np.array([[1.0, 0.0, 0.0], [0.0, np.sqrt(0.5), -np.sqrt(0.5)], [0.0, np.sqrt(0.5), np.sqrt(0.5)]])}  # pi / 4 about x


def gantry(rest_R=None):
    """A fixed base link "bed", a link "column" that slides along z (DOF 0) and on it a link "carriage" that slides along x (DOF 1): identity
    rest rotations, dyadic rest offsets -- the carriage's origin is at (0.25 + q1, 0, 0.5 + q0), one rounding a coordinate.  ``rest_R``: the
    rest rotation of the carriage (about x, so that its joint axis stays the world's x)."""
    from flobaroid_amd.topology import Topology

    R = np.tile(np.eye(3), (3, 1, 1))
    if rest_R is not None:
        R[2] = rest_R
    params = np.zeros((3, 10))
    params[:, 0] = 1.0
    params[:, [4, 7, 9]] = 0.0625
    return Topology(name="gantry", link_names=["bed", "column", "carriage"], parent=[-1, 0, 1], joint_names=["", "lift", "slide"], joint_type=[0, 2, 2],
                    dof_index=[-1, 0, 1], rest_R=R, rest_p=np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.5], [0.25, 0.0, 0.0]]),
                    axis=np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), params=params, dof_names=["lift", "slide"])


def turned_gantry(turn):
    """the gantry whose carriage carries the exact rest rotation TURNS[turn]: "apex_down" puts a cone's apex at the bottom, "on_side" lays
    a prism on a side edge (vertex 3 n / 4 of an n-gon, n a multiple of 4, has y = -r exactly), "quarter" stands a box on an edge"""
    return gantry(TURNS[turn])
