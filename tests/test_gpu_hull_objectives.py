"""collisionMode "convex" through the batched objective: candidate_objectives_from_coefficients(collision=...) with the mesh hulls of the
left arm and the crane's boxes as hulls equals the sample-by-sample restatement of the reference's collision block (main trajectory and
transitions, strict <, margins) built on the Qhull restatement (tests/test_hulls.py restate_hull_block), on the host copy of the
device-generated states -- with the base at rest and at the simulated poses of the suspended base.

Tolerance: 1e-12 max(1, largest |world coordinate|), the box block's (tests/test_gpu_box_objectives.py): the poses of the two walks differ
by roundings of the world coordinates and every distance is 1-Lipschitz in them; the hull routine's own deviation (a few eps x scale) is
far below.  Links are left out of the check (ignoreLinksForCollision) to keep the Qhull restatement at a few seconds."""
import os

import numpy as np
import pytest

import hull_restatement as hr
from common import GOLDEN, load_topo
from test_gpu_box_objectives import _cols, _host
from test_hulls import as_tuples, left_arm_hulls, restate_hull_block

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("suspended", [False, True])
def test_left_arm_mesh_hulls_under_the_crane(suspended):
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from flobaroid_amd.collision import collision_set, world_hulls_from_urdf

    topo, (hulls, box_links) = left_arm_hulls()
    assert not box_links
    eng = Engine(topo, floating=True)
    rng = np.random.default_rng(31)
    n, C, T, freq = topo.num_dofs, 3, 30, 100.0
    config = {"floatingBase": 1, "minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0, "collisionCheckStep": 3,
              "transitionDuration": 3.0, "transitionCollisionSamples": 2, "collisionMode": "convex", "worldCollisionMargin": 0.01,
              "ignoreLinksForCollision": ["Waist", "LShp", "LShr", "LWrMot2", "LWrMot3", "ground_link", "crane_column"]}
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
    if suspended:
        assert np.abs(rpy).max() > 1e-3
    # the crane moved so that its tip sits where the hand is at a checked sample of the first candidate: that pair overlaps there
    wh = world_hulls_from_urdf(os.path.join(GOLDEN, "urdf", "world_walkman_suspended.urdf"), "geometric")
    _, hand = hr.hull_world(topo, as_tuples(topo, [hulls["LSoftHandLink"]]), q[3:4], True, rpy[3:4], None if bpos is None else bpos[3:4], False)
    shift = hand[0, 0] + np.array([0.02, 0.0, 0.0]) - wh["crane_tip"].offset
    for h in wh.values():
        h.offset = h.offset + shift
    cs = collision_set(topo, {}, config, hulls=hulls, world_hulls=wh)
    P = len(cs["pair_names"])
    assert np.all(cs["columns"][:, 0] == 2) and 8 <= P <= 16 and any(b in wh for _, b in cs["pair_names"]) and any(b not in wh for _, b in cs["pair_names"])
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    cols = _cols(eng, topo, True)
    base = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, **kw)
    full = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, collision=cs, **kw)
    n0 = base["g"].shape[1]
    # without collision= nothing else changes: the same bits
    assert full["g"].shape == (C, n0 + P) and full["g"][:, :n0].tobytes() == base["g"].tobytes() and np.asarray(full["f"]).tobytes() == np.asarray(base["f"]).tobytes()
    tup = as_tuples(topo, cs["hulls"])
    _, cen = hr.hull_world(topo, tup, q, True, rpy, bpos, False)
    tol = 1e-12 * max(1.0, float(np.abs(cen).max()))
    for k in range(C):
        s = slice(k * T, (k + 1) * T)
        g, _, argmin = restate_hull_block(topo, True, cs, q[s], config, rpy[s], None if bpos is None else bpos[s])
        err = np.abs(full["g"][k, n0:] - g).max()
        print(f"candidate {k}: convex collision block max |delta| {err:.2e} (tolerance {tol:.2e}); {int((g < 0).sum())} of {P} pairs in collision")
        assert err <= tol
        assert all(full["ag_cache"]["collision_argmin_idx"][k, p] == argmin.get(p, -1) for p in range(P)), k
    blk = full["g"][:, n0:]
    assert (blk < 0).any() and (blk > 0).any()
    # without hulls the mode is refused; the gradient entry points refuse the set
    with pytest.raises(ValueError, match="needs a collision set with hulls"):
        exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config,
                                                   collision={"capsules": [], "pairs": np.zeros((0, 2))}, **kw)
    if not suspended:
        with pytest.raises(ValueError, match="hull pairs"):
            exc.candidate_gradients_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, dopt_scale=1.0, collision=cs)
    eng.close()
