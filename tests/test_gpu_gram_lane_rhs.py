"""Two rhs columns through the Gram pass over sample-contiguous images (csrc/fbr_gram64.h, option gram_lane) -- the call
Model.computeRegressors makes: rhs = [tau | contactForcesSum].

Oracle: OracleModel, A = [Y | rhs] with rhs (S rows, 2) random.  Bars: 1e-12 relative against A^T A (the bar of
test_gpu_options.py::test_gram_lane_and_force_tiles_are_switches_not_results), 1e-13 relative between the two passes of the library on
the same inputs, bitwise for symmetry, repetition and submissions.  A model outside the pass is asserted to be outside, never dropped."""
import numpy as np
import pytest

from common import load_topo, random_states, random_topology

pytestmark = pytest.mark.gpu

S0 = 64 * 9 + 37

# name, floating, friction, options, inside the pass (all 480 columns of WALK-MAN need a tile program in two parts)
NAMED = [("walkman_apriori", True, False, {"reduce_min_work": 0}, True),
         ("walkman_apriori", True, False, {"reduce_min_work": 1e30}, False),
         ("walkman_left_arm", True, False, {"reduce_min_work": 0}, True),
         ("walkman_left_arm", True, False, {"reduce_min_work": 1e30}, True),
         ("kuka_lwr4", False, False, {"reduce_min_work": 1e30}, True),
         ("walkman_left_arm", True, True, {"reduce_min_work": 1e30}, True)]
IDS = ["walkman-reduced", "walkman-direct-two-parts", "left_arm-reduced", "left_arm-direct", "kuka-fixed", "left_arm-friction"]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _engine(t, floating, fric, opts):
    from flobaroid_amd._lib import Engine

    return Engine(t, floating=floating, friction=fric, friction_symmetric=True, options=opts)


def _problem(name, floating, fric, S, seed):
    from oracle.oracle import OracleModel

    t = load_topo(name)
    om = OracleModel(t, floating=floating, fric=fric, fric_sym=True)
    rng = np.random.default_rng(seed)
    st = random_states(t, S, rng, floating, use_limits=True)
    if fric:
        st["sign"] = np.tanh(st["dq"] / 0.02)
    Y = om.regressor(st, st.get("sign"))
    rhs = rng.standard_normal((Y.shape[0], 2))
    return t, om, rng, st, Y, rhs


@pytest.mark.parametrize("name,floating,fric,opts,inside", NAMED, ids=IDS)
def test_lane_info_reports_two_rhs_columns(name, floating, fric, opts, inside):
    t = load_topo(name)
    eng = _engine(t, floating, fric, opts)
    off = _engine(t, floating, fric, dict(opts, gram_lane=0))
    try:
        assert eng.gram_lane_info(2, S0)["active"] == inside
        assert eng.gram_lane_info(1, S0)["active"] == inside and eng.gram_lane_info(0, S0)["active"] == inside
        assert not eng.gram_lane_info(3, S0)["active"]
        for k in (0, 1, 2, 3):
            assert not off.gram_lane_info(k, S0)["active"]
        if inside:
            i1, i2 = eng.gram_lane_info(1, S0), eng.gram_lane_info(2, S0)
            assert i2["mfma_per_block"] == i1["mfma_per_block"] and i2["tile_rows"] == i1["tile_rows"]  # the rhs columns have no tiles
    finally:
        eng.close()
        off.close()


@pytest.mark.parametrize("name,floating,fric,opts,inside", NAMED, ids=IDS)
def test_two_rhs_columns_match_the_oracle(name, floating, fric, opts, inside):
    """eng.gram(st, rhs) with two rhs columns: plain, row weights, base-wrench-only mask, accumulation over two calls split off a block
    boundary, several chunks, without force tiles, 16 waves, as a submission and from pinned host inputs."""
    import torch

    t, om, rng, st, Y, rhs = _problem(name, floating, fric, S0, 71)
    S, rows = S0, om.rows
    A = np.hstack([Y, rhs])
    Go = A.T @ A
    w = 0.5 + rng.random(S * rows)
    Aw = A * w[:, None]
    wb = np.zeros((S, rows))
    wb[:, :6] = 1.0 + rng.random((S, 6))
    wb = wb.reshape(-1)
    Ab = A * wb[:, None]
    h = 64 * 4 + 5
    first = {k: v[:h] for k, v in st.items()}
    second = {k: v[h:] for k, v in st.items()}
    got = {}
    variants = (("lane", {}), ("chunks", {"chunk_samples": 200}), ("no_force_tiles", {"gram_force_tiles": 0}), ("waves16", {"gram_lane_waves": 16}),
                ("images", {"gram_lane": 0}))
    for key, extra in variants:
        eng = _engine(t, floating, fric, dict(opts, **extra))
        try:
            assert eng.gram_lane_info(2, S)["active"] == (inside and key != "images"), key
            G = eng.gram(st, rhs=rhs)
            print(name, key, "rel", _rel(G, Go))
            assert _rel(G, Go) <= 1e-12, key
            assert np.array_equal(G, G.T), key
            assert np.array_equal(G, eng.gram(st, rhs=rhs)), key
            Gw = eng.gram(st, rhs=rhs, w=w)
            print(name, key, "weights rel", _rel(Gw, Aw.T @ Aw))
            assert _rel(Gw, Aw.T @ Aw) <= 1e-12 and np.array_equal(Gw, Gw.T), key
            if floating:
                Gb = eng.gram(st, rhs=rhs, w=wb)
                print(name, key, "base-only rel", _rel(Gb, Ab.T @ Ab))
                assert _rel(Gb, Ab.T @ Ab) <= 1e-12 and np.array_equal(Gb, Gb.T), key
                got[key + "_base"] = Gb
            G2 = eng.gram(second, rhs=rhs[h * rows:], out=eng.gram(first, rhs=rhs[: h * rows]), accumulate=True)
            assert _rel(G2, Go) <= 1e-12 and np.array_equal(G2, G2.T), key
            dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in st.items()}
            out = torch.zeros((om.P + 2, om.P + 2), dtype=torch.float64, device="cuda")
            eng.wait(eng.gram_submit(dev, out, rhs=torch.from_numpy(rhs).cuda()))
            assert np.array_equal(out.cpu().numpy(), G), key
            pin = {k: torch.from_numpy(np.ascontiguousarray(v)).pin_memory() for k, v in st.items()}
            prhs, pw = torch.from_numpy(rhs).pin_memory(), torch.from_numpy(w).pin_memory()
            out2 = torch.zeros_like(out)
            eng.wait(eng.gram_submit(pin, out2, rhs=prhs, w=pw))
            Gp = out2.cpu().numpy()
            print(name, key, "pinned rel", _rel(Gp, Aw.T @ Aw))
            assert _rel(Gp, Aw.T @ Aw) <= 1e-12 and np.array_equal(Gp, Gp.T), key
            got[key], got[key + "_w"], got[key + "_pin"] = G, Gw, Gp
        finally:
            eng.close()
    for key in ("lane", "chunks", "no_force_tiles", "waves16"):
        for sfx in ("", "_w", "_pin") + (("_base",) if floating else ()):
            r = _rel(got[key + sfx], got["images" + sfx])
            print(name, key + sfx, "against the image pass", r)
            assert r <= 1e-13, (key, sfx)


@pytest.mark.parametrize("name,floating,fric,opts,inside", [NAMED[0], NAMED[3], NAMED[4], NAMED[5]], ids=[IDS[0], IDS[3], IDS[4], IDS[5]])
def test_rhs_columns_are_not_mixed_up(name, floating, fric, opts, inside):
    t, om, rng, st, Y, rhs = _problem(name, floating, fric, 64 * 3 + 11, 72)
    P = om.P
    w = 0.5 + rng.random(Y.shape[0])
    eng = _engine(t, floating, fric, opts)
    try:
        assert eng.gram_lane_info(2, 64 * 3 + 11)["active"] == inside
        for second in ("scaled", "zero"):
            r = rhs.copy()
            r[:, 1] = r[:, 1] * 1e3 if second == "scaled" else 0.0
            for wt in (None, w):
                W2 = np.ones(Y.shape[0]) if wt is None else wt * wt
                G = eng.gram(st, rhs=r, w=wt)
                gn = np.linalg.norm(np.hstack([Y, r]) * np.sqrt(W2)[:, None], 2) ** 2
                for i in (0, 1):
                    assert np.linalg.norm(G[:P, P + i] - Y.T @ (W2 * r[:, i])) <= 1e-12 * gn, (second, i)
                    assert np.array_equal(G[:P, P + i], G[P + i, :P])
                    assert abs(G[P + i, P + i] - r[:, i] @ (W2 * r[:, i])) <= 1e-12 * max(r[:, i] @ (W2 * r[:, i]), 1e-300) + 0.0
                corner = r[:, 0] @ (W2 * r[:, 1])
                assert G[P, P + 1] == G[P + 1, P]
                if second == "zero":
                    assert G[P, P + 1] == 0.0 and G[P + 1, P + 1] == 0.0 and not G[:, P + 1].any()
                else:
                    assert abs(G[P, P + 1] - corner) <= 1e-12 * np.sqrt(G[P, P] * G[P + 1, P + 1])
    finally:
        eng.close()


@pytest.mark.parametrize("name,floating,fric,opts,inside", [NAMED[0], NAMED[3], NAMED[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_three_rhs_columns_and_grouped_rhs_keep_the_image_pass(name, floating, fric, opts, inside):
    """outside the scope of the lane pass: their results are the oracle's at the bars these calls have (test_gpu_fuzz.py: 1e-11)"""
    t, om, rng, st, Y, rhs = _problem(name, floating, fric, 64 * 6, 73)
    rows = om.rows
    rhs3 = np.hstack([rhs, rng.standard_normal((Y.shape[0], 1))])
    eng = _engine(t, floating, fric, opts)
    try:
        assert not eng.gram_lane_info(3, 64 * 6)["active"]
        A3 = np.hstack([Y, rhs3])
        G3 = eng.gram(st, rhs=rhs3)
        assert _rel(G3, A3.T @ A3) <= 1e-11 and np.array_equal(G3, G3.T)
        A = np.hstack([Y, rhs])
        gn = np.linalg.norm(A.T @ A)
        for ng in (2, 3):
            Gg = eng.gram_grouped(st, ng, rhs=rhs)
            hh = 64 * 6 // ng * rows
            for g in range(ng):
                Ag = A[g * hh:(g + 1) * hh]
                assert np.linalg.norm(Gg[g] - Ag.T @ Ag) <= 1e-11 * gn, (ng, g)
    finally:
        eng.close()


def test_model_compute_regressors_takes_the_lane_pass(tmp_path):
    """Model.computeRegressors (walkman_left_arm, floating base, a contact): G_aug comes from the lane pass and agrees with the same model
    on an engine with gram_lane = 0.  Which pass ran is read from the engine's profile of the call computeRegressors makes: the lane pass
    launches no kinematics-record kernel (class "kin"), the per-sample-image pass one per chunk."""
    from flobaroid_amd.data import Data
    from flobaroid_amd.model import Model
    from test_gpu_model import _opt

    path = str(tmp_path / "walkman_left_arm.topology.json")
    topo = load_topo("walkman_left_arm")
    topo.save_json(path)
    S = 400
    rng = np.random.default_rng(3)
    st = random_states(topo, S, rng, 1, use_limits=True)
    frame = list(topo.frames)[1]
    meas = {"positions": st["q"], "velocities": st["dq"], "accelerations": st["ddq"], "torques": rng.standard_normal((S, 7)),
            "base_velocity": st["base_vel"], "base_acceleration": st["base_acc"], "base_rpy": st["rpy"],
            "times": np.arange(S) / 100.0, "contacts": np.array({frame: rng.standard_normal((S, 6))})}
    res = {}
    for key, eopts in (("lane", {}), ("images", {"gram_lane": 0})):
        opt = _opt(floatingBase=1, randomSamples=1500, engineOptions=eopts)
        np.random.seed(9)
        model = Model(opt, path)
        data = Data(opt)
        data.init_from_data(meas)
        model.computeRegressors(data)
        assert np.any(model.contactForcesSum != 0.0)
        eng = model.engine
        n = data.num_used_samples
        assert eng.gram_lane_info(2, n)["active"] == (key == "lane")
        rhs = np.stack((model.tau, model.contactForcesSum), axis=1)
        eng.profile_enable(True)
        eng.profile_get()
        G = eng.gram(model._states, rhs=rhs)
        prof = eng.profile_get()
        eng.profile_enable(False)
        assert np.array_equal(G, model.G_aug)  # the call computeRegressors made, repeated: the same pass, the same bits
        assert (prof["kin"][1] == 0) == (key == "lane") and prof["pack"][1] >= 1 and prof["gram"][1] >= 1, (key, prof)
        A = np.column_stack([model.YStd, rhs])
        assert _rel(model.G_aug, A.T @ A) <= 1e-11  # (the bar of test_gpu_model.py)
        res[key] = model.G_aug
    print("G_aug lane against images", _rel(res["lane"], res["images"]))
    assert _rel(res["lane"], res["images"]) <= 1e-13


FUZZ_CASES = 32
FUZZ_SEED = 4242


def _fuzz_case(case):
    rng = np.random.default_rng([FUZZ_SEED, case])
    p = dict(L=int(rng.integers(2, 40)), floating=bool(rng.random() < 0.5), fric=bool(rng.random() < 0.4), p_fixed=float(rng.choice([0.0, 0.2, 0.5])),
             p_prism=float(rng.choice([0.0, 0.0, 0.3])), branch=float(rng.choice([0.0, 0.3, 0.7, 1.0])),
             S=int(rng.choice([1, 3, 64, 129, 500, 777, 1536])), weights=int(rng.integers(0, 3)), chunk=int(rng.choice([0, 0, 64, 200])),
             mode=str(rng.choice(["default", "reduced", "allcols"])))
    return p, rng


def _run_tree(t, p, rng, why):
    """k = 2 on tree t: the oracle's Gram at 1e-12 through whichever pass the model gets, the two passes within 1e-13 of each other
    where the lane pass serves it, symmetric and repeatable to the bit; returns whether the lane pass served it"""
    from oracle.oracle import OracleModel

    om = OracleModel(t, floating=p["floating"], fric=p["fric"], fric_sym=True)
    S, rows = p["S"], om.rows
    st = random_states(t, S, rng, p["floating"])
    if p["fric"]:
        st["sign"] = np.tanh(st["dq"] / 0.02)
    Y = om.regressor(st, st.get("sign"))
    rhs = rng.standard_normal((S * rows, 2))
    w = None
    if p["weights"]:
        w = 0.5 + rng.random(S * rows)
        if p["weights"] == 2:
            w[rng.random(S * rows) < 0.1] = 0.0
    A = np.hstack([Y, rhs]) if w is None else np.hstack([Y, rhs]) * w[:, None]
    Go = A.T @ A
    opts = {"default": {}, "reduced": {"reduce_min_work": 0}, "allcols": {"link_merge": 0}}[p["mode"]]
    if p["chunk"]:
        opts = dict(opts, chunk_samples=p["chunk"])
    eng = _engine(t, p["floating"], p["fric"], opts)
    off = _engine(t, p["floating"], p["fric"], dict(opts, gram_lane=0))
    try:
        active = bool(eng.gram_lane_info(2, S)["active"])
        assert active == bool(eng.gram_lane_info(1, S)["active"]), why  # two rhs columns wherever one is served
        assert not off.gram_lane_info(2, S)["active"], why
        G = eng.gram(st, rhs=rhs, w=w)
        assert _rel(G, Go) <= 1e-12, (why, _rel(G, Go))
        assert np.array_equal(G, G.T) and np.array_equal(G, eng.gram(st, rhs=rhs, w=w)), why
        Gi = off.gram(st, rhs=rhs, w=w)
        assert _rel(G, Gi) <= 1e-13, (why, _rel(G, Gi))
        return active
    finally:
        eng.close()
        off.close()


@pytest.mark.parametrize("case", range(FUZZ_CASES))
def test_random_trees_with_two_rhs_columns(case):
    p, rng = _fuzz_case(case)
    t = random_topology(rng, p["L"], p_fixed=p["p_fixed"], branchiness=p["branch"], p_prismatic=p["p_prism"])
    rows = t.num_dofs + (6 if p["floating"] else 0)
    if t.num_dofs == 0 or rows > 60:  # (no regressor / no tile program: not a Gram of the fused kernels at all)
        t = random_topology(rng, 12, p_fixed=0.0, branchiness=p["branch"])
    _run_tree(t, p, rng, f"FUZZ_SEED={FUZZ_SEED} case {case}: {p}")


@pytest.mark.parametrize("depth,floating,weights", [(4, True, 1), (8, False, 0), (10, True, 1), (10, False, 0), (12, False, 1), (24, True, 0),
                                                    (8, True, 1), (12, True, 0), (24, False, 1), (4, False, 0)])
def test_every_depth_instance_of_the_producer(depth, floating, weights):
    """chains of 4 / 8 / 10 / 12 / 24 joints: the depth thresholds of the producer's instances (kinimg_by_depth), with and without row
    weights -- every two-column instance of fbr_kinimg_kernel runs, on a model the lane pass serves"""
    rng = np.random.default_rng([77, depth])
    t = random_topology(rng, depth + 1, p_fixed=0.0, branchiness=0.0)
    assert t.num_dofs == depth
    p = dict(floating=floating, fric=depth == 8, S=64 * 2 + 9, weights=weights, chunk=0, mode="allcols")
    assert _run_tree(t, p, rng, f"chain of {depth} joints, floating {floating}"), "a chain is inside the lane pass"
