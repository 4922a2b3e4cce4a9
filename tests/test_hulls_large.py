"""Hulls of 129 to 1024 vertices on the CPU (csrc/fbr_hull.h, csrc/fbr_hull_large.h; DESIGN.md 8, "Large convex hulls").  Needs no GPU.

* the emulation tests/emul/hull_emul.cpp -- the text of fbr_hull_distance under g++ -ffp-contract=off -- against the Qhull restatement of
  tests/hull_restatement.py on shapes of 129 to 1024 vertices and on the hulls of KUKA LWR4's visual meshes (tests/hull_large_shapes.py):
  random poses, and contacts from 1e-2 apart to 1e-3 deep.  The rule is the file's own, 32 eps x scale (the larger of that and 10 x a
  deviation measured on the same inputs IS that, where the deviation is the quantity under test).  Among the inputs are KUKA poses on
  which a support-pair key of 8 bits -- the width before hulls above 128 vertices were served -- returns another value: the test builds
  the emulation a second time with -DFBR_HULL_KEY_BITS=8, picks them by comparing the two, and asserts that the 8-bit build misses the
  rule on every one of them.  That build has the arithmetic of the commit before (the key is the one decision that changed), so this
  test fails there: built against that header in a scratch copy of the tree, hull_emul.cpp returned the bits of the 8-bit build on all 17
  poses found here, 1.5e10 to 6.9e12 eps x scale from the restatement (0.54 mm at most; over 4000 poses a pair up to 9.4 cm).
* the largest GJK iteration count over every input of this file, asserted below FBR_HULL_MAX_ITER = 64 and recorded.
* the facet pass shared by a wave (tests/emul/hull_large_emul.cpp: 64 parts, joined in lane order with the pass's own rule) against
  fbr_hull_distance with == on every touching case, two 1024-point spheres and lwr_4_link against lwr_6_link among them.
* what fbr_model_set_large_hulls accepts and refuses, the constants in the header, collision.py and the binding, the new symbol.

Measured here: |emulation - restatement| <= 0.94 eps x scale over all inputs (random poses 0.72, contacts 0.0041, the 17 KUKA poses
0.94); the 8-bit build on the KUKA poses 1.5e10 to 6.9e12 eps x scale; most GJK iterations 15; 56 touching cases, 51 of them overlapping."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import hull_large_shapes as ls
import hull_restatement as hr
import hull_shapes as hs
from common import ROOT
from test_boxes import random_rotations
from test_hulls import EPS, GAPS, MAX_ITER, _c, _check_tables, _p, _rz, _stacked, emul_distance, tables

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "hull_large_emul.cpp")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_libs = {}


def emul_large(key_bits=None):
    """tests/emul/hull_large_emul.cpp as a library; ``key_bits`` 8: the same text with the support-pair key of before (a mutation)"""
    if key_bits not in _libs:
        out = os.path.join(_HERE, "emul", "_build", "libhull_large_emul%s.so" % ("" if key_bits is None else "_key%d" % key_bits))
        deps = [_SRC, os.path.join(ROOT, "include", "fbr.h")] + [os.path.join(_CSRC, h) for h in ("fbr_hull_large.h", "fbr_hull.h", "fbr_box.h", "fbr_capsule.h",
                                                                                                   "fbr_math.h", "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            flags = [] if key_bits is None else ["-DFBR_HULL_KEY_BITS=%d" % key_bits]
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"] + flags + ["-o", out, _SRC])
        _libs[key_bits] = ctypes.CDLL(out)
    return _libs[key_bits]


def large_distance(A, B, RA, cA, RB, cB, wave, key_bits=None):
    """(dist (N,), GJK iterations (N,), facet pass entered (N,)) of N poses; ``wave``: the facet pass as fbr_hull_large_pairs_kernel shares it"""
    vbeg, v, fbeg, pl, ebeg, ed, diam = tables([A, B])
    RA, cA, RB, cB = (_c(np.asarray(x, dtype=np.float64).reshape(len(RA), -1)) for x in (RA, cA, RB, cB))
    N = len(RA)
    out, it = np.zeros(N), np.zeros(N, dtype=np.int32)
    emul_large(key_bits).hull_large_distance(ctypes.c_long(N), _p(RA), _p(cA), _p(RB), _p(cB), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), _p(diam),
                                             int(wave), _p(out), _p(it))
    return out, it % 1000, it >= 1000


def large_parts(A, B, RA, cA, RB, cB):
    """(N, 64): the partial maxima the 64 lanes hold before they are joined"""
    vbeg, v, fbeg, pl, ebeg, ed, diam = tables([A, B])
    RA, cA, RB, cB = (_c(np.asarray(x, dtype=np.float64).reshape(len(RA), -1)) for x in (RA, cA, RB, cB))
    out = np.zeros((len(RA), 64))
    emul_large().hull_large_parts(ctypes.c_long(len(RA)), _p(RA), _p(cA), _p(RB), _p(cB), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), _p(diam), _p(out))
    return out


def test_tables_and_counts_of_the_large_shapes_and_the_kuka_fixture():
    from flobaroid_amd.collision import FBR_MAX_HULL_VERTICES, FBR_MAX_LARGE_HULL_VERTICES

    for kind in ls.KINDS:
        h = ls.shape(kind)
        _check_tables(h)
        assert (len(h.vertices), len(h.planes), len(h.edges)) == ls.COUNTS[kind], kind
    K = ls.kuka_hulls()
    for name in ls.KUKA_LINKS:
        _check_tables(K[name])
        assert (len(K[name].vertices), len(K[name].planes), len(K[name].edges)) == ls.KUKA_COUNTS[name], name
    nv = [c[0] for c in list(ls.COUNTS.values()) + list(ls.KUKA_COUNTS.values())]
    assert min(nv) == 129 > FBR_MAX_HULL_VERTICES and max(nv) == FBR_MAX_LARGE_HULL_VERTICES == 1024 and {256, 257} <= set(nv)
    z = np.load(os.path.join(ROOT, "tests", "golden", "kuka_hulls.npz"))  # data only: names, counts, float32 coordinates, offsets
    assert sorted(z.files) == ["link", "mesh", "offset", "vbeg", "verts"] and z["verts"].shape == (4154, 3) and z["offset"].shape == (8, 3)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kuka_hulls.npz")) < 64 * 1024


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
KUKA_PAIRS = (("lwr_base_link", "lwr_5_link"), ("lwr_7_link", "lwr_2_link"), ("lwr_7_link", "lwr_6_link"))
KUKA_POSES = 40  # random poses a pair among which the poses of the narrow key are looked for


def _poses_about(rng, A, B, n, lo, hi):
    """n poses: B's centre along a random direction u at lo .. hi x the sum of the two support widths along u (1: the supporting planes touch)"""
    for _ in range(n):
        RA, RB = random_rotations(rng, 2)
        u = rng.standard_normal(3)
        u /= np.linalg.norm(u)
        reach = float((A.vertices @ RA.T @ u).max() - (B.vertices @ RB.T @ u).min())
        cA = rng.standard_normal(3) * 0.3 * A.diameter
        yield RA, cA, RB, cA + u * reach * rng.uniform(lo, hi)


@functools.lru_cache(maxsize=None)
def kuka_key_poses():
    """[(A, B, RA, cA, RB, cB, tag)]: the poses among KUKA_POSES seeded ones a pair on which the emulation returns another value with a key
    of 8 bits than with the key of the header -- the comparison that found the defect"""
    K = ls.kuka_hulls()
    rng = np.random.default_rng(41)
    out = []
    for a, b in KUKA_PAIRS:
        A, B = K[a], K[b]
        P = list(_poses_about(rng, A, B, KUKA_POSES, 0.9, 1.15))
        RA, cA, RB, cB = (np.array([p[i] for p in P]) for i in range(4))
        wide, narrow = large_distance(A, B, RA, cA, RB, cB, False)[0], large_distance(A, B, RA, cA, RB, cB, False, key_bits=8)[0]
        out += [(A, B, RA[i], cA[i], RB[i], cB[i], f"{a} / {b} pose {i}: 8-bit key {narrow[i]:.6g}, header {wide[i]:.6g}") for i in np.nonzero(wide != narrow)[0]]
    return out


def random_cases():
    """every kind against itself and against the next kind (but the two slowest for Qhull, cone on cone and cone on the 1024-point sphere),
    four KUKA pairs: three poses each"""
    rng = np.random.default_rng(40)
    kinds = ("sphere129", "sphere256", "sphere257", "prism400", "prism130", "cone512", "sphere1024")
    pairs = [(k, k) for k in kinds if k != "cone512"] + [(a, b) for a, b in zip(kinds[:-2], kinds[1:-1])] + [("sphere129", "sphere1024")]
    for ka, kb in pairs:
        A, B = ls.shape(ka), ls.shape(kb)
        for j, (RA, cA, RB, cB) in enumerate(_poses_about(rng, A, B, 3, 0.8, 1.2)):
            yield A, B, RA, cA, RB, cB, f"{ka} / {kb} pose {j}"
    K = ls.kuka_hulls()
    for a, b in (("lwr_6_link", "lwr_2_link"), ("lwr_4_link", "lwr_6_link"), ("lwr_1_link", "lwr_3_link"), ("lwr_5_link", "lwr_7_link")):
        for j, (RA, cA, RB, cB) in enumerate(_poses_about(rng, K[a], K[b], 3, 0.8, 1.2)):
            yield K[a], K[b], RA, cA, RB, cB, f"{a} / {b} pose {j}"


def contact_cases():
    """B's lowest feature straight above A's highest, at the gaps of tests/test_hulls.py: a vertex of a sphere on a cap and on a sphere's
    vertex, the apex of the 511-gon cone on a cap, parallel caps of a 200-gon and a 65-gon, a 200-gon prism's side edge on a cap, KUKA's
    wrist (793 vertices) on its base"""
    down, side = hs.TURNS["apex_down"], hs.TURNS["on_side"]
    s, K = ls.shape, ls.kuka_hulls()
    kinds = {"sphere vertex on a 200-gon's cap": (s("prism400"), s("sphere257"), _rz(0.3), (0.0625, -0.03125)),
             "sphere on sphere": (s("sphere1024"), s("sphere256"), down, (0.0, 0.0)),
             "apex on a cap": (s("prism130"), s("cone512"), down, (0.0625, -0.03125)),
             "parallel caps": (s("prism400"), s("prism130"), _rz(0.3), (0.03125, -0.0625)),
             "side edge on a cap": (s("prism400"), s("prism400"), side, (0.03125, 0.0625)),
             "wrist on base": (K["lwr_base_link"], K["lwr_6_link"], _rz(0.3), (0.0, 0.0))}
    for kind, (A, B, RB, xy) in kinds.items():
        for gap in GAPS:
            yield (*_stacked(A, B, RB, xy, gap), f"{kind}, gap {gap:g}")


FAMILIES = {"large shapes, random poses": random_cases, "large shapes, contacts": contact_cases, "KUKA poses of the 8-bit key": kuka_key_poses}


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """[(case, |emulation - restatement| in eps x scale, restatement, emulation, GJK iterations, facet pass entered)] of a family, computed
    once for the tests below; the emulation is hull_emul.cpp's hull_distance"""
    out = []
    for case in FAMILIES[name]():
        A, B, RA, cA, RB, cB, tag = case
        want = hr.hull_distance(RA, cA, A.vertices, RB, cB, B.vertices)
        got, it, facet = emul_distance(A, B, RA[None], cA[None], RB[None], cB[None])
        out.append((case, abs(got[0] - want) / (EPS * hr.pair_scale(cA, A.diameter, cB, B.diameter)), want, got[0], int(it[0]), bool(facet[0])))
    return out


@pytest.mark.parametrize("name", list(FAMILIES))
def test_emulation_equals_the_restatement_on_large_hulls(name):
    """32 eps x scale on every input, the facet pass exactly where the restatement is <= 0; a third of the random poses and of the contacts
    on either side of 0.  The KUKA poses of the 8-bit key (all apart: that key ends GJK early, so its value is too large) -- see the module
    docstring: six at least, and the key of before misses the rule on every one of them."""
    res = evaluated(name)
    devs, wants = np.array([r[1] for r in res]), np.array([r[2] for r in res])
    for (case, dev, want, got, it, facet) in res:
        assert facet == (want <= 0) or abs(want) <= 64 * EPS, (case[6], want, facet)
        assert dev <= 32.0, (case[6], dev, want)
    print(f"{name}: worst |emulation - restatement| = {devs.max():.3g} eps x scale ({res[int(devs.argmax())][0][6]}); most GJK iterations "
          f"{max(r[4] for r in res)}; {(wants > 0).sum()} separated, {(wants <= 0).sum()} touching or overlapping of {len(wants)}")
    if name != "KUKA poses of the 8-bit key":
        assert 3 * (wants > 0).sum() >= len(wants) and 3 * (wants <= 0).sum() >= len(wants)
        return
    assert len(res) >= 6
    narrow = []
    for (A, B, RA, cA, RB, cB, tag), dev, want, got, it, facet in res:
        d8 = large_distance(A, B, RA[None], cA[None], RB[None], cB[None], False, key_bits=8)[0][0]
        assert d8 > want and d8 != got, tag
        narrow.append(abs(d8 - want) / (EPS * hr.pair_scale(cA, A.diameter, cB, B.diameter)))
    print(f"{len(res)} KUKA poses: the 8-bit key is {min(narrow):.3g} to {max(narrow):.3g} eps x scale from the restatement, "
          f"{max(abs(r[3] - large_distance(*r[0][:2], *(x[None] for x in r[0][2:6]), False, key_bits=8)[0][0]) for r in res):.3g} m at most from the header's key")
    assert min(narrow) > 32.0


@functools.lru_cache(maxsize=None)
def touching_cases():
    """[(A, B, RA, cA, RB, cB, tag, fbr_hull_distance's value, GJK iterations)]: every case above that enters the facet pass, two 1024-point
    spheres and lwr_4_link against lwr_6_link in overlapping poses"""
    rng = np.random.default_rng(42)
    K = ls.kuka_hulls()
    out = [(*r[0], r[3], r[4]) for name in FAMILIES for r in evaluated(name) if r[5]]
    for A, B, why in ((ls.shape("sphere1024"), ls.shape("sphere1024"), "two 1024-point spheres"), (K["lwr_4_link"], K["lwr_6_link"], "lwr_4_link / lwr_6_link")):
        for j, (RA, cA, RB, cB) in enumerate(_poses_about(rng, A, B, 6, 0.6, 0.98)):
            serial, it, facet = emul_distance(A, B, RA[None], cA[None], RB[None], cB[None])
            if facet[0]:
                out.append((A, B, RA, cA, RB, cB, f"{why}, overlapping pose {j}", serial[0], int(it[0])))
    return out


def test_the_shared_facet_pass_equals_the_serial_one():
    """fbr_hull_large_distance (64 parts in lane order, the pass's own rule, the sample's lane keeps the result) == fbr_hull_distance on every
    touching case: a maximum does not depend on how the facets are dealt out.  ==, not the bytes: the sign of a zero gap may."""
    cases = touching_cases()
    tags = " ".join(c[6] for c in cases)
    assert len(cases) >= 50 and tags.count("two 1024-point spheres") >= 4 and tags.count("lwr_4_link / lwr_6_link, overlapping") >= 4
    neg = 0
    for A, B, RA, cA, RB, cB, tag, serial, it in cases:
        wave, itw, facet = large_distance(A, B, RA[None], cA[None], RB[None], cB[None], True)
        assert facet[0] and itw[0] == it, tag
        assert wave[0] == serial, (tag, wave[0], serial)
        part = large_parts(A, B, RA[None], cA[None], RB[None], cB[None])[0]
        assert part.max() == serial and (part > -1e300).all(), tag  # (every lane has facets of its own: 64 faces or edges at least)
        neg += serial < 0
    print(f"shared facet pass: {len(cases)} touching cases equal, {neg} of them overlapping")
    assert neg >= 30


def test_gjk_iterations_stay_below_the_cap():
    """the largest GJK iteration count over every input of this file: below FBR_HULL_MAX_ITER, which stays as it is for small hulls"""
    most = max([r[4] for name in FAMILIES for r in evaluated(name)] + [c[8] for c in touching_cases()])
    print(f"most GJK iterations over the inputs of this file: {most} (the cap: {MAX_ITER})")
    assert 8 <= most < MAX_ITER
    assert 2 * most <= MAX_ITER  # (no input comes near the cap; should one, it is reported here and the cap for small hulls is not changed)


# ---- validation, constants, symbols -----------------------------------------------------------------------------------------------------------
def _validate(hull, large):
    vbeg, v, fbeg, pl, ebeg, ed, _ = tables([hull])
    link, off, rot, pairs = _c([0], np.int32), _c(np.zeros(3)), _c(np.eye(3)).reshape(-1), _c(np.zeros((0, 2)), np.int32)
    msg = ctypes.create_string_buffer(256)
    rc = emul_large().hull_large_validate(1, int(large), 1, _p(link), _p(off), _p(rot), _p(vbeg), _p(v), _p(fbeg), _p(pl), _p(ebeg), _p(ed), 0, _p(pairs), msg, 256)
    return rc, msg.value.decode()


def test_set_large_hulls_accepts_1024_vertices_and_refuses_1025():
    from flobaroid_amd.collision import Hull

    assert _validate(ls.shape("sphere1024"), True) == (0, "")
    over = Hull("over", hs.fibonacci_sphere(1025, 0.25), np.zeros(3))
    rc, msg = _validate(over, True)
    assert len(over.vertices) == 1025 and rc == -1 and "1025 vertices (4 to 1024)" in msg
    for kind, nv in (("prism130", 130), ("sphere1024", 1024)):  # fbr_model_set_hulls keeps its cap
        rc, msg = _validate(ls.shape(kind), False)
        assert rc == -1 and f"{nv} vertices (4 to 128)" in msg
    assert _validate(ls.shape("prism130"), True) == (0, "")
    assert emul_large().hull_large_key_bits() == 10 and emul_large(8).hull_large_key_bits() == 8


def test_large_hull_symbols_and_constants_in_header_binding_and_library():
    from flobaroid_amd import _lib, collision

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    name = "fbr_model_set_large_hulls"
    assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr)
    assert _lib._SIGNATURES[name] == _lib._SIGNATURES["fbr_model_set_hulls"]
    assert lib.fbr_version() == _lib.FBR_VERSION == 104
    limits = {k: int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) for k in ("FBR_MAX_HULL_VERTICES", "FBR_MAX_LARGE_HULL_VERTICES")}
    assert limits == {"FBR_MAX_HULL_VERTICES": 128, "FBR_MAX_LARGE_HULL_VERTICES": 1024}
    for mod in (collision, _lib):
        assert {k: getattr(mod, k) for k in limits} == limits, mod.__name__
    assert lib.fbr_model_set_large_hulls(None, 0, None, None, None, 0, None, None, None, None, None, None, 0, None) == -1  # FBR_E_INVALID: no model
    assert '"hull_large_all"' in hdr and "hull_large_all" in open(os.path.join(_CSRC, "fbr_options.h")).read()
    import inspect

    assert inspect.signature(_lib.Engine.set_hulls).parameters["large"].default is False


# ---- the Python layers above the binding ------------------------------------------------------------------------------------------------------
class _Recorder:
    """an engine that only records how its hull set is installed"""

    def __init__(self, strict):
        self.calls, self.strict = [], strict

    def set_hulls(self, hulls, pairs, offset_in_link_axes=False, **kw):
        if self.strict:
            assert not kw  # (the engines of before: set_hulls(hulls, pairs, offset_in_link_axes=False))
        self.calls.append(kw)
        raise _Installed


class _Installed(Exception):
    pass


def _kuka_set(links):
    from flobaroid_amd.collision import collision_set, world_hulls_from_urdf
    from common import GOLDEN, load_topo

    topo = load_topo("kuka_lwr4")
    K = ls.kuka_hulls()
    wh = world_hulls_from_urdf(os.path.join(GOLDEN, "urdf", "world_kuka.urdf"), "geometric")
    return topo, collision_set(topo, {}, {"collisionMode": "convex"}, hulls={n: K[n] for n in links}, world_hulls=wh)


def test_collision_block_installs_large_sets_with_the_keyword_and_gradients_refuse_them():
    from flobaroid_amd import excitation as exc
    from test_hulls import small_hull_set

    config = {"collisionMode": "convex", "collisionCheckStep": 1}
    topo, cs = _kuka_set(ls.KUKA_LINKS)
    assert len(cs["hull_pairs"]) > 0 and exc._large_hulls(cs)[-2:] == [("lwr_6_link", 793), ("lwr_7_link", 158)]
    eng = _Recorder(False)
    with pytest.raises(_Installed):
        exc._collision_block(eng, {"q": np.zeros((2, 7))}, 1, config, cs)
    assert eng.calls == [{"large": True}]
    _, small = small_hull_set(np.random.default_rng(5))
    eng = _Recorder(True)
    with pytest.raises(_Installed):
        exc._collision_block(eng, {"q": np.zeros((2, 2))}, 1, config, small)
    assert eng.calls == [{}] and exc._large_hulls(small) == []
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    for kw in ({}, {"hull_gradient": True}, {"box_gradient": True}, {"mesh_gradient": True}):
        with pytest.raises(ValueError, match=r"lwr_6_link \(793 vertices\)"):
            exc.candidate_collision_gradient(None, {"q": np.zeros((2, 7))}, 1, [], 50.0, config, cs, **kw)
        with pytest.raises(ValueError, match=r"lwr_6_link \(793 vertices\)"):
            exc.candidate_gradients_from_coefficients(None, [], 2, 50.0, None, None, limits, topo.dof_names, config, collision=cs, **kw)


def test_set_hulls_refuses_meshes_on_a_large_set_before_it_calls_the_library():
    from flobaroid_amd import _lib

    with pytest.raises(ValueError, match="large=True"):
        _lib.Engine.set_hulls(object(), [], [], meshes={0: np.zeros((1, 3, 3))}, large=True)
