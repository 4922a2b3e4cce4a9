"""fullMeshLinks through the batched objective: candidate_objectives_from_coefficients(collision=<set with meshes>) on the left arm, its
forearm a triangle mesh (Forearm.STL, 70 triangles), the other links their hulls and the crane's boxes as hulls, equals the
sample-by-sample restatement of the reference's collision block (main trajectory and transitions, strict <, margins) built on
tests/mesh_restatement.py (tests/test_meshes.py restate_mesh_block), on the host copy of the device-generated states -- with the base at
rest and at the simulated poses of the suspended base.

The bar, per pair: the larger of 10 x the deviation the library's own text on the CPU (tests/emul) shows against the restatement on the
block's configurations, and 32 eps x the pair's scale |cB - cA| + diam hull A + diam hull B at the winning configuration -- the bar of
tests/test_gpu_meshes.py; before the device's block is compared, every configuration of a mesh pair is asserted out of the grey zone and
the emulation's minima to lie within the bars.  Links are left out of the check (ignoreLinksForCollision) and C = 2, one transition
sample: the Qhull restatement of a triangle against a hull takes half a millisecond.
Seen on an MI355X: 1.7e-16 = 0.028 bars at rest, 1.1e-16 = 0.019 bars suspended (bars 3.5e-15 to 4.5e-15 at the least, emulation -
restatement 2.8e-16 at most); a mesh pair touches in the suspended case."""
import os

import numpy as np
import pytest

import hull_restatement as hr
from common import GOLDEN
from test_gpu_box_objectives import _cols, _host
from test_hulls import as_tuples, left_arm_hulls
from test_meshes import fixture_meshes, restate_mesh_block

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("suspended", [False, True])
def test_left_arm_with_the_forearm_as_a_mesh(suspended):
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from flobaroid_amd.collision import collision_set, world_hulls_from_urdf

    topo, (hulls, box_links) = left_arm_hulls()
    ms = fixture_meshes()
    eng = Engine(topo, floating=True)
    rng = np.random.default_rng(33)
    n, C, T, freq = topo.num_dofs, 2, 30, 100.0
    config = {"floatingBase": 1, "minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0, "collisionCheckStep": 3,
              "transitionDuration": 3.0, "transitionCollisionSamples": 1, "collisionMode": "convex", "fullMeshLinks": ["LForearm"], "worldCollisionMargin": 0.01,
              "ignoreLinksForCollision": ["Waist", "LShp", "LShr", "LElb", "LWrMot2", "LWrMot3", "ground_link", "crane_column", "crane_arm"]}
    spec = None
    if suspended:
        config["floatingBaseAttachment"] = "suspended"
        spec = {"attachment_frame": "LShy", "damping": 500.0, "x_std": topo.x_std()}
    kw = {"suspended": spec} if suspended else {}
    cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.3 for _ in range(n)], [rng.standard_normal(2) * 0.3 for _ in range(n)],
                                      rng.uniform(-0.1, 0.1, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    st = exc.candidate_states(eng, cands, T, freq, **kw)
    q = _host(st["q"])
    rpy = _host(st["rpy"]) if "rpy" in st else np.zeros((C * T, 3))
    bpos = _host(st["base_position"]) if "base_position" in st else None
    # the crane moved so that its tip sits beside the forearm at a checked sample of the first candidate
    wh = world_hulls_from_urdf(os.path.join(GOLDEN, "urdf", "world_walkman_suspended.urdf"), "geometric")
    _, arm = hr.hull_world(topo, as_tuples(topo, [hulls["LForearm"]]), q[3:4], True, rpy[3:4], None if bpos is None else bpos[3:4], False)
    shift = arm[0, 0] + np.array([0.12, 0.0, 0.0]) - wh["crane_tip"].offset
    for h in wh.values():
        h.offset = h.offset + shift
    cs = collision_set(topo, {}, config, hulls=hulls, world_hulls=wh, meshes=ms)
    P = len(cs["pair_names"])
    names = [h.link_name or h.name for h in cs["hulls"]]
    assert [names[h] for h in cs["meshes"]] == ["LForearm"] and 4 <= P <= 8 and sum("LForearm" in p for p in cs["pair_names"]) >= 3
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    cols = _cols(eng, topo, True)
    base = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, **kw)
    full = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, collision=cs, **kw)
    n0 = base["g"].shape[1]
    assert full["g"].shape == (C, n0 + P) and full["g"][:, :n0].tobytes() == base["g"].tobytes()
    meshed = np.array(["LForearm" in p for p in cs["pair_names"]])
    for k in range(C):
        s = slice(k * T, (k + 1) * T)
        g, _, argmin, bar, dev = restate_mesh_block(topo, True, cs, q[s], config, rpy[s], None if bpos is None else bpos[s], with_bar=True)
        err = np.abs(full["g"][k, n0:] - g)
        print(f"candidate {k}: mesh collision block max |delta| {err.max():.2e} = {(err / bar).max():.3f} bars (emulation - restatement {dev:.2e}, "
              f"smallest bar {bar.min():.2e}); g of the mesh pairs {g[meshed].round(4).tolist()}")
        assert np.all(err <= bar)
        assert all(full["ag_cache"]["collision_argmin_idx"][k, p] == argmin.get(p, -1) for p in range(P)), k
    # a mesh pair is never below minus its margin (the distance is never negative); collisionMode "full" with the same meshes: the same block
    blk = full["g"][:, n0:]
    assert np.all(blk[:, meshed] >= -cs["margins"][meshed])
    one = {"LForearm": ms["LForearm"]}
    cs_full = collision_set(topo, {}, dict(config, collisionMode="full", fullMeshLinks=[]), hulls=hulls, world_hulls=wh, meshes=one)
    again = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names,
                                                       dict(config, collisionMode="full", fullMeshLinks=[]), collision=cs_full, **kw)
    assert again["g"].tobytes() == full["g"].tobytes()
    # the same configuration without meshes in the set is refused; the gradient entry point refuses the set by the link's name
    plain = {k: v for k, v in cs.items() if k != "meshes"}
    with pytest.raises(ValueError, match="triangle"):
        exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, collision=plain, **kw)
    if not suspended:
        with pytest.raises(ValueError, match="LForearm"):
            exc.candidate_gradients_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, dopt_scale=1.0, collision=cs,
                                                      hull_gradient=True)
    eng.close()
