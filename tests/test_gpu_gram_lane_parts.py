"""The producer of the Gram pass over sample-contiguous images (csrc/fbr_gram64.h fbr_kinimg_kernel) under the options
gram_lane_skip_unowned (default 1: a wave forms nothing for a link it walks only as an ancestor), gram_lane_parts_cut (default 0; 1: the
tree cut for the slowest wave, ancestors included) and gram_lane_chunk_rounds (default 0; 1: chunk sizes by both kernels' grids).

Neither the image nor the order of any running sum depends on which wave writes a column, and a skipped link adds nothing, so options 0
and 1 of the first two give the same bits.  Bars: 1e-13 relative between the lane pass and the per-sample-image pass (gram_lane = 0; the
bar of test_gpu_gram_lane_rhs.py), 1e-12 against the oracle's A^T A.  gram_lane_chunk_rounds only decides for calls that need more than
one chunk of 3 GB; at the sizes of a test it must leave every bit alone (asserted), its effect on the 1 M-sample step is measured by the
benchmark's output dump."""
import numpy as np
import pytest

from common import load_topo, random_states

pytestmark = pytest.mark.gpu

# name, floating, friction, options that put the model inside the lane pass
MODELS = [("threeLinks", False, False, {"reduce_min_work": 1e30}),
          ("kuka_lwr4", False, True, {"reduce_min_work": 1e30}),
          ("walkman_left_arm", True, False, {"reduce_min_work": 1e30}),
          ("walkman_apriori", True, False, {"reduce_min_work": 0})]
IDS = [m[0] for m in MODELS]
SIZES = (1, 63, 64, 65, 129, 200)
SMAX = 210  # 3 groups x 70 samples for the grouped case


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _engine(t, floating, fric, opts):
    from flobaroid_amd._lib import Engine

    return Engine(t, floating=floating, friction=fric, friction_symmetric=True, options=opts)


_PROBLEMS = {}


def _problem(name, floating, fric):
    """states of SMAX samples, the oracle's regressor, two rhs columns, row weights and the base-wrench-only mask: computed once per model"""
    if name not in _PROBLEMS:
        from oracle.oracle import OracleModel

        t = load_topo(name)
        om = OracleModel(t, floating=floating, fric=fric, fric_sym=True)
        rng = np.random.default_rng(91)
        st = random_states(t, SMAX, rng, floating, use_limits=True)
        if fric:
            st["sign"] = np.tanh(st["dq"] / 0.02)
        Y = om.regressor(st, st.get("sign"))
        rhs = rng.standard_normal((Y.shape[0], 2))
        w = 0.5 + rng.random(Y.shape[0])
        wb = np.zeros((SMAX, om.rows))
        if floating:  # (the base wrench: the first six rows of a sample)
            wb[:, :6] = 1.0 + rng.random((SMAX, 6))
        for a in (Y, rhs, w, wb):
            a.setflags(write=False)
        _PROBLEMS[name] = (t, om, st, Y, rhs, w, wb.reshape(-1))
    return _PROBLEMS[name]


def _cases(floating):
    for S in SIZES:
        for k in (0, 1, 2):
            for wt in ("none", "rows") + (("base",) if floating else ()):
                yield S, k, wt, {}
    yield 200, 1, "rows", {"chunk_samples": 64}  # several chunks
    yield 200, 2, "none", {"chunk_samples": 64}


@pytest.mark.parametrize("name,floating,fric,opts", MODELS, ids=IDS)
def test_skip_and_cut_keep_every_bit(name, floating, fric, opts):
    t, om, st, Y, rhs, w, wb = _problem(name, floating, fric)
    rows, P = om.rows, om.P
    variants = {"default": {}, "skip0": {"gram_lane_skip_unowned": 0}, "cut1": {"gram_lane_parts_cut": 1},
                "skip0cut1": {"gram_lane_skip_unowned": 0, "gram_lane_parts_cut": 1}, "rounds1": {"gram_lane_chunk_rounds": 1},
                "images": {"gram_lane": 0}}
    engines = {}
    try:
        for extra_key, extra in (("", {}), ("chunks", {"chunk_samples": 64})):
            for key, v in variants.items():
                engines[key + extra_key] = _engine(t, floating, fric, dict(opts, **v, **extra))
        for S, k, wt, extra in _cases(floating):
            sfx = "chunks" if extra else ""
            sub = {kk: v[:S] for kk, v in st.items()}
            r = None if k == 0 else np.ascontiguousarray(rhs[: S * rows, :k])
            wv = {"none": None, "rows": w[: S * rows], "base": wb[: S * rows]}[wt]
            A = Y[: S * rows] if k == 0 else np.hstack([Y[: S * rows], r])
            if wv is not None:
                A = A * wv[:, None]
            Go = A.T @ A
            why = (name, S, k, wt, sfx)
            assert engines["default" + sfx].gram_lane_info(k, S)["active"], why
            assert not engines["images" + sfx].gram_lane_info(k, S)["active"], why
            G = {key: engines[key + sfx].gram(sub, rhs=r, w=wv) for key in variants}
            for key in ("skip0", "cut1", "skip0cut1"):
                assert np.array_equal(G[key], G["default"]), (why, key)
            # chunk sizes: the block of the columns to the bit, the rhs columns and the corner at 1e-13 of their norm
            assert np.array_equal(G["rounds1"][:P, :P], G["default"][:P, :P]), why
            if k:
                assert _rel(G["rounds1"][:, P:], G["default"][:, P:]) <= 1e-13, why
            ro, ri = _rel(G["default"], Go), _rel(G["default"], G["images"])
            print(name, S, k, wt, sfx, "oracle", ro, "image pass", ri)
            assert ro <= 1e-12, why
            assert ri <= 1e-13, why
            assert np.array_equal(G["default"], G["default"].T), why
    finally:
        for e in engines.values():
            e.close()


@pytest.mark.parametrize("name,floating,fric,opts", MODELS, ids=IDS)
def test_grouped_pass_keeps_every_bit(name, floating, fric, opts):
    """fbr_gram_grouped, 3 groups x 70 samples (every group ends in a partly filled block), with row weights"""
    t, om, st, Y, rhs, w, wb = _problem(name, floating, fric)
    rows = om.rows
    A = Y * w[:, None]
    gn = np.linalg.norm(A.T @ A)
    got = {}
    for key, v in (("default", {}), ("skip0", {"gram_lane_skip_unowned": 0}), ("cut1", {"gram_lane_parts_cut": 1}), ("images", {"gram_lane": 0})):
        eng = _engine(t, floating, fric, dict(opts, reduce_grouped_min_samples=0 if opts["reduce_min_work"] == 0 else 1e30, **v))
        try:
            got[key] = eng.gram_grouped(st, 3, w=w)
        finally:
            eng.close()
    assert np.array_equal(got["skip0"], got["default"]) and np.array_equal(got["cut1"], got["default"])
    for g in range(3):
        Ag = A[g * 70 * rows:(g + 1) * 70 * rows]
        print(name, "group", g, np.linalg.norm(got["default"][g] - Ag.T @ Ag) / gn, np.linalg.norm(got["default"][g] - got["images"][g]) / gn)
        assert np.linalg.norm(got["default"][g] - Ag.T @ Ag) <= 1e-12 * gn
        assert np.linalg.norm(got["default"][g] - got["images"][g]) <= 1e-13 * gn
