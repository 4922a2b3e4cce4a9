"""The Gram pass and the TSQR, entry by entry on the scale of each entry's own two columns (tests/colscale.py), against the long-double
Gram of the same inputs: the classes of tests/edge_reference.py one by one, at their own 24 samples and tiled to 264 (partial waves,
several waves, a chunk boundary at chunk_samples = 40).  The suite's Frobenius bars of 1e-11 stay as the coarse net; these bars are about
1e-13 at 24 samples and see a column 100 x (theta = 1e-2) or 1e4 x (theta = 1e-4) smaller than the largest on its own scale.  Every bar
comes from the reference and from CPU arithmetic (tests/test_colscale_reference.py pins them), none from the device.  Worst ratios seen on
an MI355X: DESIGN.md 2 ("Column-scaled bars")."""
import numpy as np
import pytest

import colscale as cs
import edge_reference as er
from test_gpu_edges import ROUTES as EDGE_ROUTES

pytestmark = pytest.mark.gpu

T = er.CLASS_SIZE
REDUCED = {"reduce_min_work": 0, "tsqr_group_min_samples": 1, "reduce_grouped_min_samples": 1}
# the six routes of the edge tests, and every further option of csrc/fbr_options.h that selects another Gram or TSQR kernel instance at
# these sizes (tsqr_narrow_tall decides nothing below 16 x 6 x 4 rows per wave of every CU, fbr_tsqr_shape; the remaining keys change
# where and when the same kernels run, not which)
ROUTES = dict(EDGE_ROUTES)
ROUTES.update({
    "force_tiles0": {"gram_force_tiles": 0},                         # lane pass: the force rows on the tiles of every column
    "lane_waves16": {"gram_lane_waves": 16},                         # lane pass: 16 waves of 10 accumulators
    "lane_tiling0": {"gram_lane_tiling": 0},                         # lane pass on the tile program's column tiles
    "images_shape1": {"gram_lane": 0, "gram_shape": 1},              # image pass: one workgroup per CU, 18 accumulators
    "images_shape2": {"gram_lane": 0, "gram_shape": 2},              # image pass: two per CU, 10 accumulators
    "images_orient0": {"gram_lane": 0, "gram_orient": 0},            # image pass: pairs not turned
    "rhs_tile": {"gram_rhs_tile": 1},                                # dense rhs tiles instead of the packer's moments
    "reduced_regroup0": dict(REDUCED, regroup=0),                    # reductions with the fixed links merged only
    "tsqr_groups": {"tsqr_group_min_samples": 1},                    # row groups along the tree, all columns
    "tsqr_force_group0": {"tsqr_group_min_samples": 1, "tsqr_force_group": 0},
    "tsqr_wide": {"tsqr_narrow": 0},                                 # the wide level-0 kernel and its merge tree
    "tsqr_lane_writer0": {"tsqr_lane_writer": 0},                    # kinematics kernel + workgroup-per-sample writers
    "tsqr_reorder0": {"tsqr_reorder": 0},                            # columns factorised in their own order
    "tsqr_all_factors": {"tsqr_short_call_factors": 0},              # the full number of private factors, deeper merge trees
})
CASES = [(k, r) for k in er.CONFIG_KEYS for r in ROUTES]
case_ids = [f"{k}-{r}" for k, r in CASES]


def _engine(key, route):
    from flobaroid_amd._lib import Engine

    topo, floating, friction, stribeck = er.config(key)
    return Engine(topo, floating=floating, friction=friction, friction_symmetric=True, stribeck_velocity=stribeck, options=ROUTES[route])


def _halves(key, st, rhs):
    S, rows = st["q"].shape[0], er.reference(key)["rows"]
    h = S // 2
    return (({k: np.ascontiguousarray(v[:h]) for k, v in st.items()}, np.ascontiguousarray(rhs[:h * rows])),
            ({k: np.ascontiguousarray(v[h:]) for k, v in st.items()}, np.ascontiguousarray(rhs[h * rows:])))


def _factor(R):
    assert np.all(np.tril(R, -1) == 0), "the factor is not upper triangular"
    return cs.rtr(R)


def _device_grams(eng, key):
    """what -> [G or R^T R, one per (label, Call) of colscale.device_calls(key)]"""
    names = er.reference(key)["names"]
    calls = cs.device_calls(key)
    got = {what: [] for what in calls}
    for rep in cs.SIZES:
        S = f"S={T * rep}"
        for what in ("gram k=0", "gram k=1", "gram k=2", "gram weights"):
            for _, call in calls[f"{what} {S}"]:
                st, rhs, w, _ = cs.call_states(key, call)
                got[f"{what} {S}"].append(eng.gram(st, rhs=rhs, w=w))
        for _, call in calls[f"gram accumulate {S}"]:
            st, rhs, _, _ = cs.call_states(key, call)
            (a, ra), (b, rb) = _halves(key, st, rhs)
            G = eng.gram(a, rhs=ra)
            got[f"gram accumulate {S}"].append(eng.gram(b, rhs=rb, out=G, accumulate=True))
        st, rhs, _, _ = cs.call_states(key, cs.Call(tuple(names), rep, 2))
        got[f"gram_grouped {S}"] = list(eng.gram_grouped(st, len(names), rhs=rhs))
        factors = []
        for _, call in calls[f"tsqr {S}"]:
            st, rhs, _, _ = cs.call_states(key, call)
            factors.append(eng.tsqr(st, rhs=rhs))
            got[f"tsqr {S}"].append(_factor(factors[-1]))
            (a, ra), (b, rb) = _halves(key, st, rhs)
            got[f"tsqr R_in {S}"].append(_factor(eng.tsqr(b, rhs=rb, R_in=eng.tsqr(a, rhs=ra))))
        for what in ("tsqr weights", "tsqr cols"):
            for _, call in calls[f"{what} {S}"]:
                st, rhs, w, cols = cs.call_states(key, call)
                got[f"{what} {S}"].append(_factor(eng.tsqr(st, rhs=rhs, w=w, cols=cols)))
        for i in range(len(names)):
            got[f"tsqr_merge {S}"].append(_factor(eng.tsqr_merge(factors[i], factors[(i + 1) % len(names)])))
    return got


@pytest.mark.parametrize("key,route", CASES, ids=case_ids)
def test_gram_and_tsqr_entry_by_entry_on_the_scale_of_each_column(key, route):
    """fbr_gram_accumulate (k = 0, 1, 2 rhs columns, the second 1e-6 of the first; row weights from {0, 0.5, 1, 2}; accumulated over the
    two halves), fbr_gram_grouped (groups = classes), fbr_tsqr / fbr_tsqr_cols (plain, weighted, streamed through R_in, a column subset)
    and fbr_tsqr_merge (a class and the one behind it): m_theta(G) <= 16 max over the CPU routes of m_theta + N 2^-53 at theta = 1e-2 and
    1e-4, with N the stacked rows of nonzero weight."""
    eng = _engine(key, route)
    got = _device_grams(eng, key)
    eng.close()
    over = []
    for what, calls in cs.device_calls(key).items():
        line = {th: [] for th in cs.THETAS}
        for (label, call), G in zip(calls, got[what], strict=True):
            Gref, nY = cs.reference_gram(key, call)
            assert G.shape == Gref.shape and np.isfinite(np.asarray(G, dtype=np.float64)).all(), (key, route, what, label)
            bar = cs.bar(key, call)
            for th in cs.THETAS:
                m = cs.metric(G, Gref, th, nY)
                line[th].append(f"{label}={m:.1e}/{bar[th]:.1e}")
                if not m <= bar[th]:
                    over.append((what, label, th, m, bar[th]))
        for th in cs.THETAS:
            print(f"colscale | {key} | {route} | {what} | m_{th:g}/bar | " + " ".join(line[th]))
    assert not over, (key, route, over)


LS_CASES = [(k, r) for k in cs.LS_KEYS for r in ROUTES]


@pytest.mark.parametrize("key,route", LS_CASES, ids=[f"{k}-{r}" for k, r in LS_CASES])
def test_the_tsqr_factor_solves_least_squares_like_a_householder_factor(key, route):
    """A QR, not a Cholesky: x = R[:r, :r]^-1 R[:r, r] of fbr_tsqr_cols over the independent columns of the ordinary, fast and
    hard-acceleration classes against the solution of the long-double Householder factor, e = max_j |x_j - x_ref,j| d_j / max_j |x_ref,j| d_j
    <= 16 x the e of LAPACK's QR on the oracle's double matrix.  A factor of Cholesky quality is 100 x to 3000 x off in the fast and
    hard-acceleration classes (tests/test_colscale_reference.py) and fails."""
    eng = _engine(key, route)
    res = {}
    for cls in cs.LS_CLASSES:
        ls = cs.ls_case(key, cls)
        st, rhs, _, _ = cs.call_states(key, cs.Call((cls,), 1, 1))
        R = eng.tsqr(st, rhs=rhs, cols=ls["cols"])
        assert np.all(np.tril(R, -1) == 0)
        res[cls] = (cs.ls_error(cs.solve_factor(R, ls["cols"].size), ls["x_ref"], ls["d"]), cs.LS_FACTOR * ls["e_qr"], ls["e_chol"])
    eng.close()
    print(f"colscale | {key} | {route} | least squares | e/bar (e_chol) | " + " ".join(f"{c}={e:.1e}/{b:.1e} ({ch:.1e})" for c, (e, b, ch) in res.items()))
    for cls, (e, b, _) in res.items():
        assert e <= b, (key, route, cls, e, b)
