"""The rhs moments of the Gram pass over sample-contiguous images, summed over the lanes of a producer wave in registers
(csrc/fbr_mom_lanes.h, fbr_kinimg_kernel): one atomic per (part, link, rhs column), lane fbr_gram64_mom_lane(p) carrying parameter p.

What can go wrong is the partly filled last block -- the lanes behind the last sample run on that sample and must add nothing -- and
a lane adding to the wrong column.  So: sample counts that put the last block's live lanes at both sides of every half-wave boundary,
one and two rhs columns, no weights and row weights with zeros, on a floating chain of 4 joints (all ten parameters of the base link),
chains of 10 and 12 joints (the register-bound instance of the producer and the next one), WALK-MAN reduced (masked parameters: their
lanes stay off) and the left arm with friction columns.

Oracle: OracleModel, computed once per model for the largest sample count; a smaller count takes its first samples.  Bars: the rhs
rows / columns / corner at 1e-12 ||A||_2^2 (the form of test_gpu_gram_lane_rhs.py::test_rhs_columns_are_not_mixed_up), bitwise
repetition, chunks of 64 samples against one chunk at 1e-13 relative, a zero second rhs column gives an exactly zero column of G."""
import numpy as np
import pytest

from common import load_topo, random_states, random_topology

pytestmark = pytest.mark.gpu

SAMPLES = [1, 2, 31, 32, 33, 63, 64, 65, 64 * 2 + 33]
SMAX = max(SAMPLES)

# name or chain depth, floating, friction, options
MODELS = [(4, True, False, {"link_merge": 0}), (10, True, False, {"link_merge": 0}), (12, False, False, {"link_merge": 0}),
          ("walkman_apriori", True, False, {"reduce_min_work": 0}), ("walkman_left_arm", True, True, {"reduce_min_work": 1e30})]
IDS = ["floating-chain-4", "chain-10", "chain-12", "walkman-reduced", "left_arm-friction"]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _engine(t, floating, fric, opts):
    from flobaroid_amd._lib import Engine

    return Engine(t, floating=floating, friction=fric, friction_symmetric=True, options=opts)


@pytest.mark.parametrize("model,floating,fric,opts", MODELS, ids=IDS)
def test_moments_summed_over_the_wave(model, floating, fric, opts):
    from oracle.oracle import OracleModel

    rng = np.random.default_rng([311, [m[0] for m in MODELS].index(model)])
    if isinstance(model, int):
        t = random_topology(rng, model + 1, p_fixed=0.0, branchiness=0.0)
        assert t.num_dofs == model
    else:
        t = load_topo(model)
    om = OracleModel(t, floating=floating, fric=fric, fric_sym=True)
    P, rows = om.P, om.rows
    st = random_states(t, SMAX, rng, floating, use_limits=not isinstance(model, int))
    if fric:
        st["sign"] = np.tanh(st["dq"] / 0.02)
    Y = om.regressor(st, st.get("sign"))
    rhs = rng.standard_normal((SMAX * rows, 2))
    rhs[:, 1] *= 1e3  # (columns of very different scale: a mix-up shows)
    w = 0.5 + rng.random(SMAX * rows)
    w[rng.random(SMAX * rows) < 0.1] = 0.0
    eng = _engine(t, floating, fric, opts)
    chk = _engine(t, floating, fric, dict(opts, chunk_samples=64))
    try:
        for S in SAMPLES:
            sub = {k: v[:S] for k, v in st.items()}
            Ys = Y[: S * rows]
            for k in (1, 2):
                assert eng.gram_lane_info(k, S)["active"], "the model is inside the lane pass"
                for wt in (None, w[: S * rows]):
                    why = (S, k, wt is not None)
                    r = rhs[: S * rows, :k]
                    W2 = np.ones(S * rows) if wt is None else wt * wt
                    G = eng.gram(sub, rhs=r, w=wt)
                    gn = np.linalg.norm(np.hstack([Ys, r]) * np.sqrt(W2)[:, None], 2) ** 2
                    for i in range(k):
                        assert np.linalg.norm(G[:P, P + i] - Ys.T @ (W2 * r[:, i])) <= 1e-12 * gn, (why, i)
                        assert np.array_equal(G[:P, P + i], G[P + i, :P]), (why, i)
                        tt = r[:, i] @ (W2 * r[:, i])
                        assert abs(G[P + i, P + i] - tt) <= 1e-12 * max(tt, 1e-300), (why, i)
                    if k == 2:
                        assert G[P, P + 1] == G[P + 1, P], why
                        assert abs(G[P, P + 1] - r[:, 0] @ (W2 * r[:, 1])) <= 1e-12 * np.sqrt(G[P, P] * G[P + 1, P + 1]), why
                    assert np.array_equal(G, eng.gram(sub, rhs=r, w=wt)), why  # bitwise repetition
                    Gc = chk.gram(sub, rhs=r, w=wt)
                    assert _rel(Gc, G) <= 1e-13, (why, _rel(Gc, G))
                    if k == 2:  # the common contactForcesSum = 0: nothing of the first column leaks into the second
                        r0 = r.copy()
                        r0[:, 1] = 0.0
                        G0 = eng.gram(sub, rhs=r0, w=wt)
                        assert not G0[:, P + 1].any() and not G0[P + 1, :].any(), why
                        assert np.array_equal(G0[: P + 1, : P + 1], G[: P + 1, : P + 1]), why
    finally:
        eng.close()
        chk.close()
