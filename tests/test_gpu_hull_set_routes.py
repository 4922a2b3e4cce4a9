"""Which pair of a hull set goes to which kernel (csrc/fbr_collision_api.hip; DESIGN.md, "Hull set: classes, views, stencils"): every route
of fbr_candidate_hull_distances, fbr_mesh_distance_gradients and fbr_large_hull_distance_gradients at the smallest shapes that reach it.

The gantry of tests/hull_shapes.py with a box and a tetrahedron (small), the sphere of 129 vertices of tests/hull_large_shapes.py (big) and a
hull that carries a soup of 40 triangles; six pairs in the column order mesh, small, big, small, mesh, big, so that no class has contiguous
columns, the second mesh pair with its mesh on the second member.  2 candidates of 65 samples (one full tile and one lane) at step 1 -- once
more with chunk_samples = 64 (several launches), once more with one sample a candidate.  There is no reference here but the library
itself: a pair's column in an installation has the bytes of that pair installed alone through the same setters and options, whatever the
other pairs of the set make of the views and tables; and attachments come and go without a trace."""
import functools

import numpy as np
import pytest

import hull_large_shapes as hl
import hull_shapes as hs
import mesh_large_shapes as ml
from test_gpu_boxes import _engine, _host
from test_gpu_meshes import call, same

pytestmark = pytest.mark.gpu
C = 2
VARIANTS = {"T65": (65, None), "T65-chunk64": (65, {"chunk_samples": 64}), "T1": (1, None)}


@functools.lru_cache(maxsize=None)
def large_set():
    """hulls, {hull: triangles}, pairs of the set of set_hulls(large=True): 0 box, 1 tetrahedron, 2 sphere129, 3 the meshed hull"""
    from flobaroid_amd.collision import Hull

    soup = ml.soup(9, 40, 0.06)
    hulls = [Hull("column", hs.box([0.0625, 0.125, 0.0625]), np.array([0.0, 0.5, 0.0])), Hull("carriage", hs.tetra(np.random.default_rng(3), 0.15), np.array([0.0, -0.25, 0.1])),
             hl.on(hl.shape("sphere129"), "bed", [-1.0, 0.75, 0.0]), ml.hull_of(soup, "bed", offset=[0.75, 0.25, 0.25])]
    pairs = np.array([(3, 0), (0, 1), (2, 1), (1, 0), (1, 3), (0, 2)], dtype=np.int32)  # mesh, small, big, small, mesh (swap), big
    return hulls, {3: soup}, pairs


@functools.lru_cache(maxsize=None)
def small_set():
    """the small hulls alone, for set_hulls and small meshes: 0 box, 1 tetrahedron, 2 the meshed hull; mesh, small, small, mesh (swap)"""
    hulls, meshes, _ = large_set()
    return [hulls[0], hulls[1], hulls[3]], {2: meshes[3]}, np.array([(2, 0), (0, 1), (1, 0), (1, 2)], dtype=np.int32)


def states(T):
    rng = np.random.default_rng(70 + T)
    return {"q": np.ascontiguousarray(np.stack([rng.uniform(0.05, 0.3, C * T), rng.uniform(-0.2, 0.2, C * T)], axis=1))}


def picks(T, P):
    """sample on the last sample, one entry at -1, one pose_sample differing (T = 1 has no other sample)"""
    sample = np.full((C, P), T - 1, dtype=np.int64)
    sample[1, 2] = -1
    pose = sample.copy()
    pose[0, P - 1] = 0
    return sample, pose


def grads_same(a, b):
    return a["dist"].tobytes() == b["dist"].tobytes() and a["grad_q"].tobytes() == b["grad_q"].tobytes()


def column(got, k):
    return {key: np.ascontiguousarray(v[:, k:k + 1]) for key, v in got.items()}


INSTALLATIONS = {  # name -> (the set, set_hulls' keywords but the meshes, with meshes, hull_large_all)
    "large": (large_set, {"large": True}, False, 0), "large, all": (large_set, {"large": True}, False, 1),
    "large, tree meshes": (large_set, {"large": True, "large_meshes": True}, True, 0),
    "large, tree meshes, all": (large_set, {"large": True, "large_meshes": True}, True, 1),
    "small, meshes": (small_set, {}, True, 0)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_pair_in_a_set_has_the_bytes_of_the_pair_alone(variant):
    T, options = VARIANTS[variant]
    st = states(T)
    eng = _engine(hs.gantry(), False, options=options)
    for name, (the_set, kw, with_meshes, all_large) in INSTALLATIONS.items():
        hulls, meshes, pairs = the_set()
        eng.set_option("hull_large_all", all_large)
        eng.set_hulls(hulls, pairs, meshes=meshes if with_meshes else None, **kw)
        whole = call(eng, st, None, C, 1, True)
        assert same(whole, call(eng, st, None, C, 1, False)) and np.isfinite(whole["dist"]).all(), name
        for k in range(len(pairs)):
            eng.set_hulls(hulls, pairs[k:k + 1], meshes=meshes if with_meshes else None, **kw)
            assert same(column(whole, k), call(eng, st, None, C, 1, True)), (name, k)
    # the meshes matter: a mesh pair is not its hulls' pair; option hull_large_all does not change a value
    hulls, meshes, pairs = large_set()
    eng.set_option("hull_large_all", 0)
    eng.set_hulls(hulls, pairs, large=True)
    plain = call(eng, st, None, C, 1, True)
    eng.set_hulls(hulls, pairs, large=True, meshes=meshes, large_meshes=True)
    tree = call(eng, st, None, C, 1, True)
    assert np.all(tree["dist"][:, [0, 4]] > plain["dist"][:, [0, 4]]) and tree["dist"][:, [1, 2, 3, 5]].tobytes() == plain["dist"][:, [1, 2, 3, 5]].tobytes()
    eng.set_option("hull_large_all", 1)
    other = call(eng, st, None, C, 1, True)  # (the values: the sign of a zero gap may depend on the kernel)
    assert np.array_equal(tree["dist"], other["dist"]) and np.array_equal(tree["idx"], other["idx"])
    eng.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_pair_in_a_set_has_the_gradient_bytes_of_the_pair_alone(variant):
    T, options = VARIANTS[variant]
    st = states(T)
    eng = _engine(hs.gantry(), False, options=options)
    # fbr_mesh_distance_gradients on the small set with meshes
    hulls, meshes, pairs = small_set()
    sample, pose = picks(T, len(pairs))
    eng.set_hulls(hulls, pairs, meshes=meshes)
    whole = _host(eng.mesh_distance_gradients(st, C, sample, pose_sample=pose))
    assert np.isfinite(whole["grad_q"]).all() and np.any(whole["grad_q"][:, [0, 3]] != 0.0) and not whole["grad_q"][1, 2].any()
    for k in range(len(pairs)):
        eng.set_hulls(hulls, pairs[k:k + 1], meshes=meshes)
        alone = eng.mesh_distance_gradients(st, C, sample[:, k:k + 1], pose_sample=pose[:, k:k + 1])  # (k = 1, 2: a set without a mesh pair)
        assert grads_same(column(whole, k), _host(alone)), ("mesh", k)
    # fbr_large_hull_distance_gradients on the large set, hull_large_all 0 and 1, hull_grad_tile 0 and 1
    hulls, meshes, pairs = large_set()
    sample, pose = picks(T, len(pairs))
    first = None
    for all_large in (0, 1):
        for tile in (0, 1):
            eng.set_option("hull_large_all", all_large)
            eng.set_option("hull_grad_tile", tile)
            eng.set_hulls(hulls, pairs, large=True)
            whole = _host(eng.large_hull_distance_gradients(st, C, sample, pose_sample=pose))
            assert np.isfinite(whole["grad_q"]).all() and whole["grad_q"].any() and not whole["grad_q"][1, 2].any()
            first = first or whole
            assert np.array_equal(whole["dist"], first["dist"]) and np.array_equal(whole["grad_q"], first["grad_q"])  # (neither option changes a value)
            for k in range(len(pairs)):
                eng.set_hulls(hulls, pairs[k:k + 1], large=True)
                alone = eng.large_hull_distance_gradients(st, C, sample[:, k:k + 1], pose_sample=pose[:, k:k + 1])
                assert grads_same(column(whole, k), _host(alone)), (all_large, tile, k)
    eng.close()


def test_attachments_come_and_go_without_a_trace():
    from flobaroid_amd._lib import FbrError

    T = 65
    st = states(T)
    eng = _engine(hs.gantry(), False)
    hulls, meshes, pairs = small_set()
    sample, pose = picks(T, len(pairs))
    eng.set_hulls(hulls, pairs)
    bare_d, bare_g = call(eng, st, None, C, 1, True), _host(eng.hull_distance_gradients(st, C, sample, pose_sample=pose))
    # attached, then detached by an empty list: the bytes from before
    eng.set_hull_meshes(meshes)
    with_d, with_g = call(eng, st, None, C, 1, True), _host(eng.mesh_distance_gradients(st, C, sample, pose_sample=pose))
    assert not same(with_d, bare_d) and with_d["dist"][:, [1, 2]].tobytes() == bare_d["dist"][:, [1, 2]].tobytes()
    assert with_g["grad_q"][:, [1, 2]].tobytes() == bare_g["grad_q"][:, [1, 2]].tobytes()
    eng.set_hull_meshes({})
    assert same(call(eng, st, None, C, 1, True), bare_d) and grads_same(_host(eng.hull_distance_gradients(st, C, sample, pose_sample=pose)), bare_g)
    with pytest.raises(FbrError, match="has no triangle meshes attached"):
        eng.mesh_distance_gradients(st, C, sample)
    # a refused attachment (a triangle outside its hull) leaves distances and gradients as they were -- without meshes and with them
    outside = {2: meshes[2] * 3.0}
    with pytest.raises(FbrError, match="code -1"):
        eng.set_hull_meshes(outside)
    assert same(call(eng, st, None, C, 1, True), bare_d) and grads_same(_host(eng.hull_distance_gradients(st, C, sample, pose_sample=pose)), bare_g)
    eng.set_hull_meshes(meshes)
    for setter in (eng.set_hull_meshes, eng.set_large_hull_meshes):
        with pytest.raises(FbrError, match="code -1"):
            setter(outside)
        assert same(call(eng, st, None, C, 1, True), with_d) and grads_same(_host(eng.mesh_distance_gradients(st, C, sample, pose_sample=pose)), with_g)
    # a refused set_hulls (a pair of a hull with itself: refused by the checks, before anything is cleared) leaves the set AND its meshes
    # in place
    with pytest.raises(FbrError, match="code -1"):
        eng.set_hulls(hulls, np.array([(0, 1), (1, 1)], dtype=np.int32))
    assert eng.num_hull_pairs == len(pairs)
    assert same(call(eng, st, None, C, 1, True), with_d) and grads_same(_host(eng.mesh_distance_gradients(st, C, sample, pose_sample=pose)), with_g)
    # a later set_hulls drops the meshes
    eng.set_hulls(hulls, pairs)
    assert same(call(eng, st, None, C, 1, True), bare_d) and grads_same(_host(eng.hull_distance_gradients(st, C, sample, pose_sample=pose)), bare_g)
    # the large set: tree meshes attached and detached, the gradients of the large hulls served again with the bytes from before
    hulls, meshes, pairs = large_set()
    sample, pose = picks(T, len(pairs))
    eng.set_hulls(hulls, pairs, large=True)
    bare_d, bare_g = call(eng, st, None, C, 1, True), _host(eng.large_hull_distance_gradients(st, C, sample, pose_sample=pose))
    eng.set_large_hull_meshes(meshes)
    assert not same(call(eng, st, None, C, 1, True), bare_d)
    with pytest.raises(FbrError, match="attached by fbr_model_set_large_hull_meshes"):
        eng.large_hull_distance_gradients(st, C, sample)
    eng.set_large_hull_meshes({})
    assert same(call(eng, st, None, C, 1, True), bare_d) and grads_same(_host(eng.large_hull_distance_gradients(st, C, sample, pose_sample=pose)), bare_g)
    eng.close()
