"""The box pairs through the batched objective: candidate_objectives_from_coefficients(collision=...) with a set that has boxes --
collisionMode "box", and capsule mode with a world and a capsule-less link -- equals the sample-by-sample restatement of the reference's
collision block (tests/box_collision_restatement.py) on the host copy of the device-generated states, transitions included, also at the
simulated poses of the suspended base; the gradient entry points refuse such a set.

Tolerance: 1e-12 max(1, largest |world coordinate|), the capsule block's (tests/test_gpu_capsules.py): the poses of the two walks differ by
roundings of the world coordinates and every distance is 1-Lipschitz in them.  The winning sample may differ only between samples whose
restated distances are closer than that (a link rigidly attached to the fixed base keeps its distance to the world)."""
import os

import numpy as np
import pytest

import box_restatement as br
import capsule_restatement as cr
from box_collision_restatement import index_boxes, restate_mixed_block
from common import GOLDEN, load_topo, random_states
from test_boxes import kuka_mixed_set, synthetic_boxes

pytestmark = pytest.mark.gpu


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _cols(eng, topo, floating):
    import scipy.linalg as sla

    R, piv = sla.qr(eng.gram(random_states(topo, 2000, np.random.default_rng(1), floating, use_limits=True)), pivoting=True, mode="r")
    d = np.abs(np.diag(R))
    return np.sort(piv[: int((d > 1e-8 * d[0]).sum())])


def _check_block(topo, floating, cs, config, full, n0, st, C, T):
    q = _host(st["q"])
    rpy = _host(st["rpy"]) if floating else None
    bpos = _host(st["base_position"]) if floating and "base_position" in st else None
    R, c, h = br.box_world(topo, index_boxes(topo, cs["boxes"]), q, floating, rpy, bpos, bool(cs.get("center_in_link_axes", False)))
    tol = 1e-12 * max(1.0, float(np.abs(c).max()))
    P, step = len(cs["pair_names"]), config["collisionCheckStep"]
    for k in range(C):
        s = slice(k * T, (k + 1) * T)
        g, argmin, main = restate_mixed_block(topo, floating, cs, q[s], config, None if rpy is None else rpy[s], None if bpos is None else bpos[s])
        err = np.abs(full["g"][k, n0:] - g).max()
        print(f"candidate {k}: collision block max |delta| {err:.2e} (tolerance {tol:.2e}); {int((g < 0).sum())} of {P} pairs in collision")
        assert err <= tol
        got = full["ag_cache"]["collision_argmin_idx"][k]
        for p in range(P):
            ref = argmin.get(p, -1)
            if got[p] != ref:
                assert got[p] >= 0 and ref >= 0 and got[p] % step == 0 and abs(main[got[p] // step, p] - main[ref // step, p]) <= tol, (k, p, got[p], ref)
    return tol


@pytest.mark.parametrize("mode,link_axes", [("box", False), ("capsule", True)])
def test_kuka_over_the_floor(mode, link_axes):
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine

    rng = np.random.default_rng(12)
    topo, cs = kuka_mixed_set(mode, rng, link_axes=link_axes)
    assert set(cs["columns"][:, 0]) == ({0, 1} if mode == "capsule" else {1}) and any(b.link_name is None for b in cs["boxes"])
    eng = Engine(topo, floating=False)
    n, C, T, freq = topo.num_dofs, 3, 90, 50.0
    cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.4 for _ in range(n)], [rng.standard_normal(2) * 0.4 for _ in range(n)],
                                      rng.uniform(-0.2, 0.2, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    config = {"collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 4, "collisionMode": mode}
    cols = _cols(eng, topo, False)
    base = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, dopt_scale=1.0)
    full = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, dopt_scale=1.0, collision=cs)
    P = len(cs["pair_names"])
    assert full["g"].shape == (C, 5 * n + P) and np.array_equal(full["g"][:, :5 * n], base["g"]) and np.array_equal(full["f"], base["f"])
    st = exc.candidate_states(eng, cands, T, freq, device=True)
    _check_block(topo, False, cs, config, full, 5 * n, st, C, T)
    blk = full["g"][:, 5 * n:]
    assert (blk < 0).any() and (blk > 0).any()
    # the gradient entry points refuse a set with box pairs, and the mesh modes stay refused
    gcfg = dict(config, collisionMode="capsule")
    with pytest.raises(ValueError, match="box pairs"):
        exc.candidate_collision_gradient_from_coefficients(eng, cands, T, freq, gcfg, cs)
    with pytest.raises(ValueError, match="box pairs"):
        exc.candidate_gradients_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, gcfg, dopt_scale=1.0, collision=cs)
    for bad in ("convex", "full"):
        with pytest.raises(ValueError):
            exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, dict(config, collisionMode=bad),
                                                       dopt_scale=1.0, collision=cs)
    eng.close()


def test_left_arm_swinging_under_the_crane():
    """capsule mode, a capsule on every link, the four boxes of world_walkman_suspended.urdf: the robot pairs go to the capsules, the world
    pairs to the boxes, both at the simulated poses of the suspended base"""
    from flobaroid_amd import excitation as exc
    from flobaroid_amd._lib import Engine
    from flobaroid_amd.collision import Box, Capsule, collision_set, world_boxes_from_urdf

    topo = load_topo("walkman_left_arm")
    eng = Engine(topo, floating=True)
    rng = np.random.default_rng(31)
    n, C, T, freq = topo.num_dofs, 3, 48, 100.0
    names = list(topo.link_names)
    caps = {names[l]: Capsule(names[l], p0, p1, r) for l, p0, p1, r in cr.synthetic_capsules(topo)}
    boxes = {names[l]: Box(names[l], h, c) for l, h, c, _ in synthetic_boxes(topo, rng, pad=(0.08, 0.2))}
    wb = world_boxes_from_urdf(os.path.join(GOLDEN, "urdf", "world_walkman_suspended.urdf"), "geometric")
    # the crane moved so that its tip hangs 10 cm beside the origin, where the arm's base starts: the swing decides what touches
    shift = np.array([0.1, 0.0, 0.0]) - wb["crane_tip"].center
    for b in wb.values():
        b.center = b.center + shift
    config = {"floatingBase": 1, "floatingBaseAttachment": "suspended", "minVelocityConstraint": True, "minVelocityPercentage": 0.1,
              "trajectoryTargetVelocity": 1.0, "collisionCheckStep": 3, "transitionDuration": 3.0, "transitionCollisionSamples": 4,
              "collisionMode": "capsule", "worldCollisionMargin": 0.01}
    cs = collision_set(topo, caps, config, boxes=boxes, world_boxes=wb)
    assert set(cs["columns"][:, 0]) == {0, 1}
    cands = [exc.fourier_coefficients([rng.standard_normal(2) * 0.2 for _ in range(n)], [rng.standard_normal(2) * 0.2 for _ in range(n)],
                                      rng.uniform(-0.1, 0.1, n), [2] * n, wf=float(rng.uniform(0.8, 1.2))) for _ in range(C)]
    spec = {"attachment_frame": "LShy", "damping": 500.0, "x_std": topo.x_std()}
    limits = {j: dict(topo.limits[j]) for j in topo.dof_names}
    cols = _cols(eng, topo, True)
    base = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, suspended=spec)
    full = exc.candidate_objectives_from_coefficients(eng, cands, T, freq, topo.x_std(), cols, limits, topo.dof_names, config, collision=cs, suspended=spec)
    n0, P = base["g"].shape[1], len(cs["pair_names"])
    assert full["g"].shape == (C, n0 + P) and np.array_equal(full["g"][:, :n0], base["g"]) and np.array_equal(full["f"], base["f"])
    st = exc.candidate_states(eng, cands, T, freq, suspended=spec)
    assert np.abs(_host(st["rpy"])).max() > 1e-3
    _check_block(topo, True, cs, config, full, n0, st, C, T)
    world = np.array([b in wb for _, b in cs["pair_names"]])
    assert world.any() and (full["g"][:, n0:][:, world] < 0).any() and (full["g"][:, n0:][:, world] > 0).any()
    eng.close()
