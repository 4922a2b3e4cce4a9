"""The fused kernels at their size and option limits, against the CPU oracle in fp64.

The parity, options and fuzz modules run a few hundred samples with default chunking on robots of at most 60 regressor rows, options
fixed when the Engine is created.  This module goes past those limits, one case each:
  A. a lane-pass chunk whose sample-contiguous image exceeds 4 GiB (option chunk_samples above the memory cap);
  B. every option that decides which kernels run or how they are tiled, set after the first calls instead of at creation;
  C. a robot of more than 105 DOF, whose staged states do not fit the LDS of the one-lane-per-sample kernels;
  D. more than 65 535 groups of one or two samples in one fbr_gram_grouped call (the grid's y limit);
  E. joint paths on both sides of every depth that selects a register-stack instance (4 / 8 / 10 / 12 / 24) and of the switch to the
     two-kernel path above 24, through every kernel family that has such instances: the fused kinematics + torques, the Gram producer,
     the TSQR lane writer and the finite-difference sweep."""
import math

import numpy as np
import pytest

from common import load_topo, random_states, random_topology

pytestmark = pytest.mark.gpu

FBR_E_HIP = -3


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _maxabs_rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1.0))


def _joint_depth(topo):
    """Deepest joint path: the most moving joints on the way from the base to a link (what fbr_kinid_build turns into kinid.maxlvl)."""
    depth = [0] * topo.num_links
    for l in topo.traversal():
        p = topo.parent[l]
        depth[l] = (depth[p] if p >= 0 else 0) + (1 if topo.dof_index[l] >= 0 and p >= 0 else 0)
    return max(depth)


# ---------------------------------------------------------------------------------------------------------------------------------
# A. oversized lane-pass chunk
# ---------------------------------------------------------------------------------------------------------------------------------
def test_chunk_samples_above_the_image_cap_is_clamped():
    """chunk_samples asks for one chunk whose block image is > 1.15 * 2^32 bytes.  The producer's image offsets are 32-bit: the pass must
    cut the call at its memory cap anyway, and return the oracle's Gram -- bitwise the Gram of the same engine without the option."""
    import time

    from flobaroid_amd._lib import Engine
    from oracle.oracle import OracleModel

    t = load_topo("walkman_apriori")
    eng = Engine(t, floating=True, options={"reduce_min_work": 0})
    blk = eng.gram_lane_info(1, 1 << 20)["block_image_bytes"]
    assert blk > 0
    S = int(math.ceil(1.15 * 2**32 / blk)) * 64 + 17  # (a last block the producer fills partly)
    assert (S + 63) // 64 * blk >= 1.15 * 2**32
    info = eng.gram_lane_info(1, S)
    assert info["active"] and info["block_image_bytes"] == blk
    rng = np.random.default_rng(71)
    st = random_states(t, S, rng, True, use_limits=True)
    om = OracleModel(t, floating=True)
    x_std = t.x_std() * (1.0 + 0.1 * rng.standard_normal(10 * t.num_links))
    tau = om.inverse_dynamics(st, x_std).reshape(-1, 1)
    eng.set_option("chunk_samples", S)
    assert eng.gram_lane_info(1, S)["active"]
    G = eng.gram(st, rhs=tau)
    eng.set_option("chunk_samples", 0)
    G_default = eng.gram(st, rhs=tau)
    eng.close()
    t0 = time.perf_counter()
    Gu, threads = om.stack_gram(st, x_std, threads=16)
    print(f"stack_gram reference: {S} samples, {threads} threads, {time.perf_counter() - t0:.1f} s")
    Go = np.triu(Gu) + np.triu(Gu, 1).T
    assert _rel(G, Go) <= 1e-12, _rel(G, Go)
    assert np.array_equal(G, G_default)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. options set after the first call
# ---------------------------------------------------------------------------------------------------------------------------------
# (key, value other than the default): every option that changes which kernels run or how they are tiled
LATE_OPTIONS = [
    ("gram_lane", 0), ("gram_force_tiles", 0), ("gram_lane_waves", 16), ("link_merge", 0), ("regroup", 0), ("reduce_min_work", 0),
    ("chunk_samples", 200), ("tsqr_force_group", 0), ("tsqr_groups", 0), ("tsqr_lane_writer", 0), ("gram_shape", 2),
    ("reduce_grouped_min_samples", 1), ("tsqr_group_min_samples", 1), ("fused_id", 0),
]
# Options of every engine of case B but the key under test: the column reductions and the row groups of the TSQR at a few hundred
# samples, so that the keys read only on those paths (regroup, tsqr_*, reduce_grouped_min_samples) decide something
LATE_BASE = {"reduce_min_work": 0, "tsqr_group_min_samples": 1}


def _infos(eng, S, ngr):
    out = {}
    for k in (0, 1):
        out[f"lane{k}"] = eng.gram_lane_info(k, S)
        out[f"lane{k}_group"] = eng.gram_lane_info(k, S // ngr)
        out[f"program{k}"] = eng.gram_program_info(k, S)
        out[f"tsqr{k}"] = eng.tsqr_work_info(S, k)
    out["merge"] = eng.link_merge_info(S)
    return out


@pytest.mark.parametrize("key,val", LATE_OPTIONS, ids=[k for k, _ in LATE_OPTIONS])
def test_an_option_set_after_the_first_calls_takes_effect(key, val):
    """Engine A is created with the value, engine B without it; B runs every pass once and then gets the value through set_option.  The
    info calls and the kernel launches of every pass agree, and B's next passes are bitwise A's and the oracle's.  On at least one of
    the two robots A differs from an engine without the value (infos, launches or bits), so the key decides something here."""
    from flobaroid_amd._lib import Engine
    from oracle.oracle import OracleModel

    base = {k: v for k, v in LATE_BASE.items() if k != key}
    effect = {}
    for name in ("walkman_left_arm", "walkman_apriori"):
        t = load_topo(name)
        om = OracleModel(t, floating=True)
        rng = np.random.default_rng(72)
        S, ngr = 64 * 6 + 21, 3
        st = random_states(t, S, rng, True, use_limits=True)
        Y = om.regressor(st)
        tau = rng.standard_normal((Y.shape[0], 1))
        A = np.hstack([Y, tau])
        Go, G0o = A.T @ A, Y.T @ Y
        h = S // ngr * om.rows
        Ggo = [Y[g * h:(g + 1) * h].T @ Y[g * h:(g + 1) * h] for g in range(ngr)]
        x = rng.standard_normal(om.P)
        pred_o = (Y @ x).reshape(S, om.rows)
        calls = {"G": lambda e: e.gram(st, rhs=tau), "G0": lambda e: e.gram(st), "Gg": lambda e: e.gram_grouped(st, ngr),
                 "R": lambda e: e.tsqr(st, rhs=tau), "pred": lambda e: e.predict(st, x)}

        def run(eng):
            out = {}
            eng.profile_enable(True)
            eng.profile_get()
            for what, f in calls.items():
                out[what] = f(eng)
                out[what + "_launches"] = np.array([v[1] for v in eng.profile_get().values()])  # (per class; the times are not compared)
            eng.profile_enable(False)
            return out

        a = Engine(t, floating=True, options=dict(base, **{key: val}))
        b = Engine(t, floating=True, options=base)
        c = Engine(t, floating=True, options=base)
        run(b)
        b.set_option(key, val)
        assert b.get_option(key) == val
        ia, ib, ic = _infos(a, S, ngr), _infos(b, S, ngr), _infos(c, S, ngr)
        assert ib == ia, (name, key)
        ra, rb, rc = run(a), run(b), run(c)
        for what in ra:
            assert np.array_equal(ra[what], rb[what]), (name, key, what)
        effect[name] = [w for w in ("infos",) if ia != ic] + [w for w in ra if not np.array_equal(ra[w], rc[w])]
        assert _rel(rb["G"], Go) <= 1e-12, (name, key, _rel(rb["G"], Go))
        assert _rel(rb["G0"], G0o) <= 1e-12, (name, key)
        for g in range(ngr):
            assert _rel(rb["Gg"][g], Ggo[g]) <= 1e-12, (name, key, g)
        R = rb["R"]
        assert np.all(np.tril(R, -1) == 0) and _rel(R.T @ R, Go) <= 1e-12, (name, key, _rel(R.T @ R, Go))
        assert _maxabs_rel(rb["pred"], pred_o) <= 1e-11, (name, key)
        for e in (a, b, c):
            e.close()
    print(f"{key}={val}: differs from an engine without it in {effect}")
    assert any(effect.values()), (key, effect)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. many DOF
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused_or_equal(call, ref, tol, what):
    """Either the oracle's numbers, or a refusal that names the limit -- never a raw HIP error."""
    from flobaroid_amd._lib import FbrError

    try:
        got = call()
    except FbrError as e:
        msg = str(e)
        assert f"(code {FBR_E_HIP})" not in msg, (what, msg)
        assert "(code -4)" in msg and ("at most" in msg or "too large" in msg or "limited to" in msg), (what, msg)  # FBR_E_UNSUPPORTED
        print(f"{what}: refused: {msg}")
        return None
    r = ref()
    assert _rel(got, r) <= tol, (what, _rel(got, r))
    return got


def test_more_than_105_dof_fall_back_to_the_two_kernel_path():
    """~130 links on a shallow tree: n >= 110 DOF (the q / dq / ddq of a 64-sample block exceed the LDS of the one-lane-per-sample
    kernels) with joint paths within FBR_KINID_MAXD, so the fused route is the one the size rules out."""
    from flobaroid_amd._lib import Engine
    from oracle.oracle import OracleModel

    rng = np.random.default_rng(73)
    t = random_topology(rng, 130, p_fixed=0.0, branchiness=1.0)
    n = t.num_dofs
    assert n >= 110 and _joint_depth(t) <= 24
    S = 64 * 3 + 5
    st = random_states(t, S, rng, True)
    st["sign"] = np.tanh(st["dq"] / 0.02)
    for fric in (False, True):
        om = OracleModel(t, floating=True, fric=fric)
        eng = Engine(t, floating=True, friction=fric)
        assert not eng.gram_lane_info(0, S)["active"] and not eng.gram_lane_info(1, S)["active"]
        x_std = np.concatenate([t.x_std(), rng.random(om.P - 10 * t.num_links)])
        tau = eng.inverse_dynamics(st, x_std)
        tau_o = om.inverse_dynamics(st, x_std, st["sign"] if fric else None)
        assert _maxabs_rel(tau, tau_o) <= 1e-11, (fric, _maxabs_rel(tau, tau_o))
        x = rng.standard_normal(om.P)
        Yo = om.regressor(st, st["sign"] if fric else None)
        pred_o = (Yo @ x).reshape(S, om.rows)
        assert _maxabs_rel(eng.predict(st, x), pred_o) <= 1e-11, fric
        wr = rng.standard_normal((S, 6))
        for link in (t.link_names[-1], t.link_names[int(rng.integers(1, t.num_links))]):
            ct, ct_o = eng.contact_torques(st, link, wr), om.contact_torques(st, link, wr)
            assert _maxabs_rel(ct, ct_o) <= 1e-11, (fric, link)
        _refused_or_equal(lambda: eng.regressor(st), lambda: Yo, 1e-12, "regressor")
        _refused_or_equal(lambda: eng.gram(st), lambda: Yo.T @ Yo, 1e-11, "gram")
        _refused_or_equal(lambda: (lambda R: R.T @ R)(eng.tsqr(st)), lambda: Yo.T @ Yo, 1e-11, "tsqr")
        # the handle is still usable after a refusal
        assert _maxabs_rel(eng.inverse_dynamics(st, x_std), tau_o) <= 1e-11
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# D. many groups
# ---------------------------------------------------------------------------------------------------------------------------------
def test_more_groups_than_the_grid_holds():
    """fbr_gram_grouped with 70 001 groups of one or two samples on the lane route: the groups go in launches of at most 32 768 grid
    rows.  Every group checked against its own oracle Gram around the chunk edges and at random, and the sum against the whole Gram."""
    from flobaroid_amd._lib import Engine
    from oracle.oracle import OracleModel

    t = load_topo("threeLinks")
    om = OracleModel(t)
    eng = Engine(t)
    ngr = 70_001
    blk = eng.gram_lane_info(0, 2)["block_image_bytes"]
    assert eng.gram_lane_info(0, 2)["active"] and 0 < blk and blk * 65_536 < 3 * 2**30
    rng = np.random.default_rng(74)
    st = random_states(t, 2 * ngr, rng, False)
    Y = om.regressor(st)
    rows, P = om.rows, om.P
    picks = np.unique(np.concatenate([np.arange(64), np.arange(ngr - 64, ngr), np.arange(32_768 - 8, 32_768 + 8),
                                      np.arange(65_535 - 8, 65_535 + 8), rng.integers(0, ngr, 256)]))
    for Sg, weighted in ((2, False), (1, True)):
        S = Sg * ngr
        sts = {k: v[:S] for k, v in st.items()}
        Ys = Y[: S * rows]
        w = 0.5 + rng.random(S * rows) if weighted else None
        A = Ys if w is None else Ys * w[:, None]
        eng.profile_enable(True)
        eng.profile_get()
        Gg = eng.gram_grouped(sts, ngr, w=w)
        prof = eng.profile_get()
        eng.profile_enable(False)
        assert prof["kin"][1] == 0 and prof["pack"][1] >= 2, prof  # the lane route (no kinematics records), several launches
        assert Gg.shape == (ngr, P, P)
        Go = A.T @ A
        assert _rel(Gg.sum(axis=0), Go) <= 1e-12, (Sg, _rel(Gg.sum(axis=0), Go))
        Ag = A.reshape(ngr, Sg * rows, P)[picks]
        Gpo = np.einsum("gri,grj->gij", Ag, Ag)
        for i, g in enumerate(picks):
            assert _rel(Gg[g], Gpo[i]) <= 1e-12, (Sg, int(g))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# E. depth thresholds of the register-stack instances
# ---------------------------------------------------------------------------------------------------------------------------------
DEPTHS = [4, 5, 8, 9, 10, 11, 12, 13, 24, 25]


def _tree_of_depth(rng, depth, branched):
    """A main chain of `depth` joints from the base (one of them prismatic) and, when branched, side branches of random length hung off
    it that never go deeper, plus a link welded to one of them -- deepest joint path exactly `depth`."""
    from flobaroid_amd.topology import Topology

    parent, jtype, jd = [-1], [0], [0]  # jd: joints on the path
    for i in range(depth):
        parent.append(i)
        jtype.append(2 if i == depth // 2 else 1)
        jd.append(i + 1)
    if branched:
        for _ in range(3):
            a = int(rng.integers(0, len(parent)))
            while jd[a] >= depth:
                a = parent[a]
            for _ in range(int(rng.integers(1, min(depth - jd[a], 3) + 1))):
                parent.append(a)
                jtype.append(1)
                jd.append(jd[a] + 1)
                a = len(parent) - 1
                if rng.random() < 0.5:
                    break
        parent.append(int(rng.integers(1, len(parent))))
        jtype.append(0)
        jd.append(jd[parent[-1]])
    L = len(parent)
    dof, n = [], 0
    for l in range(L):
        dof.append(n if (l > 0 and jtype[l] != 0) else -1)
        n += 1 if (l > 0 and jtype[l] != 0) else 0
    rest_R = np.stack([np.eye(3)] + [np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(L - 1)])
    rest_p = rng.standard_normal((L, 3)) * 0.2
    rest_p[0] = 0
    axis = rng.standard_normal((L, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    axis[[l for l in range(L) if dof[l] < 0]] = 0
    params = np.zeros((L, 10))
    params[:, 0] = 1 + rng.random(L)
    params[:, 1:4] = 0.1 * rng.standard_normal((L, 3))
    params[:, [4, 7, 9]] = 0.05 + 0.05 * rng.random((L, 3))
    return Topology(name="depth", link_names=[f"l{l}" for l in range(L)], parent=parent, joint_names=[""] + [f"jt{l}" for l in range(1, L)],
                    joint_type=jtype, dof_index=dof, rest_R=rest_R, rest_p=rest_p, axis=axis, params=params,
                    dof_names=[f"j{d}" for d in range(n)])


@pytest.mark.parametrize("branched", [False, True], ids=["chain", "tree"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_joint_paths_at_the_instance_thresholds(depth, branched):
    from flobaroid_amd._lib import Engine
    from oracle.oracle import OracleModel

    rng = np.random.default_rng([75, depth, int(branched)])
    t = _tree_of_depth(rng, depth, branched)
    assert _joint_depth(t) == depth and 2 in t.joint_type
    floating = bool((depth + int(branched)) % 2)
    om = OracleModel(t, floating=floating)
    # (the Gram on the regrouped model: the larger trees need more than one part of the tile program over all their columns, which the
    # lane pass does not take; the TSQR by row groups at this size, the path of the lane writer)
    eng = Engine(t, floating=floating, options={"reduce_min_work": 0, "tsqr_group_min_samples": 1})
    S = 64 * 3 + 5
    st = random_states(t, S, rng, floating)
    rows, P = om.rows, om.P
    why = f"depth {depth} {'tree' if branched else 'chain'} floating={floating} L={t.num_links} n={t.num_dofs}"
    try:
        Yo = om.regressor(st)
        assert _maxabs_rel(eng.regressor(st), Yo) <= 1e-11, why
        rhs = rng.standard_normal((S * rows, 1))
        A = np.hstack([Yo, rhs])
        for k in (0, 1):
            info = eng.gram_lane_info(k, S)
            assert info["active"] == (depth <= 24), (why, k, info)
            G = eng.gram(st, rhs=rhs if k else None)
            Go = A.T @ A if k else Yo.T @ Yo
            assert _rel(G, Go) <= 1e-12, (why, k, _rel(G, Go))
        ngr = 5
        Sg = S // ngr
        Gg = eng.gram_grouped({kk: v[: ngr * Sg] for kk, v in st.items()}, ngr)
        for g in range(ngr):
            Yg = Yo[g * Sg * rows:(g + 1) * Sg * rows]
            assert _rel(Gg[g], Yg.T @ Yg) <= 1e-12, (why, "group", g)
        eng.profile_enable(True)
        eng.profile_get()
        R = eng.tsqr(st, rhs=rhs)
        prof = eng.profile_get()
        eng.profile_enable(False)
        assert np.all(np.tril(R, -1) == 0) and _rel(R.T @ R, A.T @ A) <= 1e-12, (why, _rel(R.T @ R, A.T @ A))
        # the regressor rows of the factorisation come from the lane writer (fbr_kinwrite_kernel: kinematics fused, no kinematics launch)
        # wherever the tree has more than one row group -- a floating base or a branch -- and a joint path within FBR_KINID_MAXD; a chain
        # on a fixed base is one group and keeps the plain path, deeper trees the kinematics kernel + writers
        lane_writer = depth <= 24 and (floating or branched)
        assert prof["regressor"][1] >= 1 and (prof["kin"][1] == 0) == lane_writer, (why, prof)
        x = rng.standard_normal(P)
        assert _maxabs_rel(eng.predict(st, x), (Yo @ x).reshape(S, rows)) <= 1e-11, why
        wr = rng.standard_normal((S, 6))
        for link in sorted({t.link_names[depth], t.link_names[-1]}):
            assert _maxabs_rel(eng.contact_torques(st, link, wr), om.contact_torques(st, link, wr)) <= 1e-11, (why, link)
        Sf = 11
        sf = {kk: v[:Sf] for kk, v in st.items()}
        W = rng.standard_normal((Sf * rows, P))
        eps = 1e-6
        sc = eng.fd_scores(sf, W, eps)
        n = t.num_dofs
        Wb = W.reshape(Sf, rows, P)
        ref = np.empty_like(sc)
        ref[:, 0] = np.einsum("src,src->s", Wb, Yo[: Sf * rows].reshape(Sf, rows, P))
        for kind, key in enumerate(("q", "dq", "ddq")):
            for d in range(n):
                sp = {kk: v.copy() for kk, v in sf.items()}
                sp[key][:, d] += eps
                ref[:, 1 + kind * n + d] = np.einsum("src,src->s", Wb, om.regressor(sp).reshape(Sf, rows, P))
        assert _maxabs_rel(sc, ref) <= 1e-11, why
    finally:
        eng.close()
