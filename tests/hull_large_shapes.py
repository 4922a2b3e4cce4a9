"""Shapes for the tests of hulls above FBR_MAX_HULL_VERTICES (tests/test_hulls_large.py, tests/test_gpu_hulls_large.py): round and flat
polytopes of 129 to 1024 vertices -- the first size above the small cap, the sizes on either side of 256, where a support pair's key of 8
bits begins to repeat, and the large cap itself -- and the hulls of KUKA LWR4's visual meshes from tests/golden/kuka_hulls.npz.  They ride on
the gantry of tests/hull_shapes.py, whose poses are exact.

Counts (vertices / merged faces / edges), asserted by tests/test_hulls_large.py: fibonacci_sphere(n) n / 2 n - 4 / 3 n - 6 for n = 129, 256,
257, 1024; prism(200) 400 / 202 / 600; cone(511) 512 / 512 / 1022; prism(65) 130 / 67 / 195, the smallest large hull; KUKA: KUKA_COUNTS."""
import functools
import os

import numpy as np

import hull_shapes as hs
from common import GOLDEN

KINDS = ("sphere129", "sphere256", "sphere257", "sphere1024", "prism400", "cone512", "prism130")
COUNTS = {"sphere129": (129, 254, 381), "sphere256": (256, 508, 762), "sphere257": (257, 510, 765), "sphere1024": (1024, 2044, 3066),
          "prism400": (400, 202, 600), "cone512": (512, 512, 1022), "prism130": (130, 67, 195)}
KUKA_LINKS = ("lwr_base_link", "lwr_1_link", "lwr_2_link", "lwr_3_link", "lwr_4_link", "lwr_5_link", "lwr_6_link", "lwr_7_link")
KUKA_COUNTS = {"lwr_base_link": (216, 316, 530), "lwr_1_link": (606, 1182, 1786), "lwr_2_link": (613, 1194, 1805), "lwr_3_link": (607, 1185, 1790),
               "lwr_4_link": (614, 1197, 1809), "lwr_5_link": (547, 1060, 1605), "lwr_6_link": (793, 1481, 2272), "lwr_7_link": (158, 196, 352)}


def points(kind):
    """(V, 3): sizes of a few decimetres, as the links of an arm"""
    return {"sphere129": lambda: hs.fibonacci_sphere(129, 0.25), "sphere256": lambda: hs.fibonacci_sphere(256, 0.25),
            "sphere257": lambda: hs.fibonacci_sphere(257, 0.25), "sphere1024": lambda: hs.fibonacci_sphere(1024, 0.25),
            "prism400": lambda: hs.prism(200, 0.25, 0.5), "cone512": lambda: hs.cone(511, 0.25, 0.5), "prism130": lambda: hs.prism(65, 0.25, 0.5)}[kind]()


@functools.lru_cache(maxsize=None)
def shape(kind, link="shape"):
    """the flobaroid_amd.collision.Hull of ``kind`` on ``link`` at the link's origin (built once: the tables of 1024 vertices take seconds)"""
    from flobaroid_amd.collision import Hull

    return Hull(link, points(kind), np.zeros(3))


def on(h, link, offset=None, rot=None, name=None):
    """the hull ``h`` on another link (None: a world hull with ``rot``) at ``offset``: the tables are shared, not derived again"""
    import copy

    g = copy.copy(h)
    g.link_name, g.offset, g.rot, g.name = link, np.zeros(3) if offset is None else np.asarray(offset, dtype=np.float64), rot, name
    return g


@functools.lru_cache(maxsize=None)
def kuka_hulls():
    """{link: Hull} of the eight KUKA LWR4 links from the fixture: the vertices of the hulls of the visual meshes (unscaled STL float32) and
    the offsets flobaroid_amd.collision.hulls_from_urdf gives them"""
    from flobaroid_amd.collision import Hull

    z = np.load(os.path.join(GOLDEN, "kuka_hulls.npz"))
    assert tuple(str(n) for n in z["link"]) == KUKA_LINKS and z["verts"].dtype == np.float32
    return {str(n): Hull(str(n), z["verts"][z["vbeg"][i]:z["vbeg"][i + 1]].astype(np.float64), z["offset"][i]) for i, n in enumerate(z["link"])}
