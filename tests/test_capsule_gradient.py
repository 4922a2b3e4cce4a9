"""The capsule distance gradient off the GPU: the NumPy restatement (tests/capsule_gradient_restatement.py) is held against central
differences of the distance restatement, the HIP-free text of csrc/fbr_capsule_grad.h (g++, tests/emul/capsule_grad_emul.cpp) against the
restatement, the chain restatement against central differences of the series, and the C-ABI carries the two new entry points under 104."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import capsule_gradient_restatement as cg
import capsule_restatement as cr
import fourier_gradient_restatement as frest
from common import ROOT, load_topo, random_states, random_topology

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "capsule_grad_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libcapsule_grad_emul.so")
_CSRC = os.path.join(ROOT, "flobaroid_amd", "csrc")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lib = None
EPS = 1e-6


def emul():
    global _lib
    if _lib is None:
        deps = [_SRC] + [os.path.join(_CSRC, h) for h in ("fbr_capsule_grad.h", "fbr_capsule.h", "fbr_math.h", "fbr_kinid.h", "fbr_program.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, _SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def emul_items(topo, floating, capsules, item_pairs, q, rpy=None, base_pos=None):
    """(dist (M,), grad (M, n)) from the library's own walk and item routine on the CPU"""
    c = lambda a, t=np.float64: np.ascontiguousarray(a, dtype=t)  # noqa: E731
    parent, dof, jt = c(topo.parent, np.int32), c(topo.dof_index, np.int32), c(topo.joint_type, np.int32)
    rR, rp, ax = c(topo.rest_R).reshape(-1), c(topo.rest_p).reshape(-1), c(topo.axis).reshape(-1)
    link = c([k[0] for k in capsules], np.int32)
    seg = c([np.concatenate([k[1], k[2]]) for k in capsules]).reshape(-1)
    rad = c([k[3] for k in capsules])
    pr = c(item_pairs, np.int32).reshape(-1)
    q = c(q)
    M = q.shape[0]
    rpy = None if rpy is None else c(rpy)
    bp = None if base_pos is None else c(base_pos)
    dist, grad = np.zeros(M), np.full((M, topo.num_dofs), np.nan)
    rc = emul().capgrad_eval(topo.num_links, topo.num_dofs, parent.ctypes.data_as(_ip), dof.ctypes.data_as(_ip), _d(rR), _d(rp), _d(ax),
                             jt.ctypes.data_as(_ip), int(floating), len(capsules), link.ctypes.data_as(_ip), _d(seg), _d(rad), ctypes.c_long(M),
                             pr.ctypes.data_as(_ip), _d(q), _d(rpy), _d(bp), _d(dist), _d(grad))
    assert rc == 0
    return dist, grad


def shifted_capsules(topo, rng, radius=0.03):
    """a capsule on every link with both end points moved off the link's origin (the lever arm of a closest point never degenerates to the
    link origin); every third one is a sphere"""
    caps = []
    for i, (l, p0, p1, _) in enumerate(cr.synthetic_capsules(topo, radius)):
        a = p0 + rng.standard_normal(3) * 0.05
        caps.append((l, a, a.copy() if i % 3 == 2 else p1 + rng.standard_normal(3) * 0.05, radius))
    return caps


def cases():
    """(name, topology, floating, capsules, pairs, q, rpy, base_pos): the robots of the issue, S = 20 configurations each"""
    out = []
    for k, (name, fl) in enumerate((("threeLinks", False), ("kuka_lwr4", False), ("walkman_left_arm", False), ("kuka_lwr4", True), ("random", False))):
        rng = np.random.default_rng(100 + k)
        topo = random_topology(rng, 14, p_fixed=0.25, branchiness=0.5, p_prismatic=0.3) if name == "random" else load_topo(name)
        caps = shifted_capsules(topo, rng)
        pairs = cr.non_neighbour_pairs(topo, caps)
        if len(pairs) == 0:  # (threeLinks: a chain of three, its only non-neighbours may be missing)
            pairs = np.array([(i, j) for i in range(len(caps)) for j in range(i + 1, len(caps))], dtype=np.int32)
        S = 20
        q = random_states(topo, S, rng, False, use_limits=name != "random")["q"]
        rpy = rng.uniform(-np.pi, np.pi, (S, 3)) if fl else None
        bp = rng.standard_normal((S, 3)) if fl else None
        out.append((f"{name}-fb{int(fl)}", topo, fl, caps, pairs, q, rpy, bp))
    return out


CASES = cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_central_differences(case):
    """|restatement - central difference (eps = 1e-6)| <= 1e-8: the rounding floor of the difference quotient is ulp(1) / eps ~ 1e-10, the
    wrong lever-arm sign is off by 0.05 .. 0.8.  An item is left out only where ``near`` is set or the branch code at q +- eps e_j differs
    from the one at q; at most 5 % of the items."""
    name, topo, fl, caps, pairs, q, rpy, bp = case
    ref = cg.distance_gradient(topo, caps, pairs, q, fl, rpy, bp)
    S, P, n = ref["grad"].shape
    fd = np.zeros((S, P, n))
    skip = np.repeat(ref["near"][..., None], n, axis=2)
    for j in range(n):
        side = []
        for sgn in (1.0, -1.0):
            qq = q.copy()
            qq[:, j] += sgn * EPS
            d = cr.capsule_distances(cr.capsule_world(topo, caps, qq, fl, rpy, bp), caps, pairs)
            skip[..., j] |= d["branch"] != ref["branch"]
            side.append(d["dist"])
        fd[..., j] = (side[0] - side[1]) / (2 * EPS)
    share = skip.mean()
    err = np.abs(ref["grad"] - fd)[~skip].max()
    print(f"{name}: max |grad - FD| = {err:.3e} over {int((~skip).sum())} entries, left out {100 * share:.2f} %, max |grad| = {np.abs(ref['grad']).max():.3f}")
    assert share <= 0.05
    assert err <= 1e-8
    assert np.abs(ref["grad"]).max() > 0.05  # (the case exercises the lever arms at all)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_library_text_equals_the_restatement(case):
    """the g++ build of fbr_capgrad_item: per item |delta grad| <= 1e-12 max(1, world scale) parameter_condition, the distance to 1e-12
    max(1, world scale), joints off the pair's path exactly 0.0"""
    name, topo, fl, caps, pairs, q, rpy, bp = case
    ref = cg.distance_gradient(topo, caps, pairs, q, fl, rpy, bp)
    assert not ref["near"].any()
    S, P, n = ref["grad"].shape
    rep = lambda a: None if a is None else np.repeat(a, P, axis=0)  # noqa: E731
    dist, grad = emul_items(topo, fl, caps, np.tile(pairs, (S, 1)), rep(q), rep(rpy), rep(bp))
    dist, grad = dist.reshape(S, P), grad.reshape(S, P, n)
    tol = cg.gradient_tolerance(ref)
    errd, errg = np.abs(dist - ref["dist"]).max(), (np.abs(grad - ref["grad"]).max(axis=2) / tol).max()
    print(f"{name}: max |delta dist| = {errd:.3e} (tolerance {1e-12 * ref['scale']:.1e}), max |delta grad| / tolerance = {errg:.3f}")
    assert errd <= 1e-12 * ref["scale"]
    assert np.all(np.abs(grad - ref["grad"]).max(axis=2) <= tol)
    assert np.all(grad[~ref["on_path"]] == 0.0)
    assert ref["on_path"].any() and (~ref["on_path"]).any() or n < 3


def test_library_text_corner_rules():
    """coincident closest points: a zero row and the distance -r_a - r_b; two capsules on one link: a zero row; a NaN configuration: NaN in
    the distance and the path joints, zeros elsewhere"""
    topo = load_topo("kuka_lwr4")
    rng = np.random.default_rng(5)
    caps = shifted_capsules(topo, rng)
    l3, l6 = caps[3][0], caps[6][0]
    q = random_states(topo, 1, rng, False, use_limits=True)["q"]
    # a sphere on link 6 and a sphere on link 3 placed, at this q, on the very same world point
    from np_dynamics import world_kinematics

    z = np.zeros((1, 3))
    kin = world_kinematics(topo, q, 0 * q, 0 * q, np.eye(3)[None], z, z, z, z)
    w = kin["R"][l6, 0] @ np.array([0.0, 0.0, 0.1]) + kin["p"][l6, 0]
    local3 = kin["R"][l3, 0].T @ (w - kin["p"][l3, 0])
    caps = caps + [(l6, np.array([0.0, 0.0, 0.1]), np.array([0.0, 0.0, 0.1]), 0.02), (l3, local3, local3.copy(), 0.03),
                   (l3, np.array([0.1, 0, 0]), np.array([0.1, 0, 0.2]), 0.01)]
    n0 = len(caps) - 3
    dist, grad = emul_items(topo, False, caps, [[n0, n0 + 1], [n0 + 1, n0 + 2], [0, 6]], np.repeat(q, 3, axis=0))
    ref = cg.item_gradients(topo, caps, [[n0, n0 + 1]], q)
    assert abs(dist[0] + 0.05) <= 1e-12 and np.all(grad[0] == 0.0) and np.all(ref["grad"] == 0.0)  # (|p_A - p_B| ~ 1e-16 < 1e-12)
    assert np.all(grad[1] == 0.0) and np.isfinite(dist[1])
    assert np.abs(grad[2]).max() > 0
    qn = q.copy()
    qn[0, 1] = np.nan
    dist, grad = emul_items(topo, False, caps, [[0, 6]], qn)
    on = cg.path_dofs(topo, caps[0][0], caps[6][0])
    assert np.isnan(dist[0]) and np.all(np.isnan(grad[0][on])) and np.all(grad[0][~on] == 0.0)


@pytest.mark.parametrize("bounded", [False, True], ids=["classic", "bounded"])
def test_chain_restatement_equals_central_differences_of_the_series(bounded):
    """f(p) = scale sum_d g_d q_d(t; p) at t = sample / freq, sample 0, a middle one and T - 1, scale != 1: the chain row against central
    differences (eps = 1e-6) in every variable, wf included.  Bar 1e-7: the quotient's rounding floor is sum|g| ulp(|q| <= 8) / eps ~ 1e-8
    for n = 5 joints and the truncation eps^2 / 6 |f'''| stays below 1e-8 for t <= 0.6 s and three harmonics; entries are of order 0.1 .. 1."""
    rng = np.random.default_rng(8 + bounded)
    n, nh, T, freq = 5, 3, 7, 10.0
    A, B = rng.standard_normal((n, nh)) * 0.4, rng.standard_normal((n, nh)) * 0.4
    wf, qoff = 1.3, rng.uniform(-0.3, 0.3, n)
    qr = rng.uniform(0.5, 1.5, n) if bounded else None
    sample = np.array([0, 3, T - 1, -1])
    scale = np.array([0.7, 0.25, 0.9, 0.5])
    g = rng.standard_normal((4, n))
    got = cg.position_chain(wf, qr, A, B, sample, scale, g, freq)
    assert np.all(got[3] == 0)

    def f(wf_, qoff_, qr_, A_, B_, r):
        t = np.array([sample[r] / freq])
        return scale[r] * sum(g[r, d] * frest.series(wf_, qoff_[d], None if qr_ is None else qr_[d], A_[d], B_[d], t)[0][0] for d in range(n))

    def fd(r, kind, j=0, l=0):
        v = []
        for sgn in (1.0, -1.0):
            w_, o_, r_, A_, B_ = wf, qoff.copy(), None if qr is None else qr.copy(), A.copy(), B.copy()
            if kind == "wf":
                w_ = wf + sgn * EPS
            elif kind == "off":
                o_[j] += sgn * EPS
            elif kind == "rng":
                r_[j] += sgn * EPS
            elif kind == "a":
                A_[j, l] += sgn * EPS
            else:
                B_[j, l] += sgn * EPS
            v.append(f(w_, o_, r_, A_, B_, r))
        return (v[0] - v[1]) / (2 * EPS)

    worst = 0.0
    for r in range(3):
        want = np.zeros_like(got[r])
        want[0] = fd(r, "wf")
        for j in range(n):
            want[1 + j] = fd(r, "off", j)
            want[1 + n + j] = fd(r, "rng", j) if bounded else 0.0
            for l in range(nh):
                want[1 + 2 * n + j * nh + l] = fd(r, "a", j, l)
                want[1 + 2 * n + n * nh + j * nh + l] = fd(r, "b", j, l)
        worst = max(worst, np.abs(got[r] - want).max())
        assert np.abs(got[r] - want).max() <= 1e-7, (r, np.abs(got[r] - want).max())
        assert np.abs(got[r]).max() > 0.05
    print(f"chain restatement, bounded={bounded}: max |chain - FD| = {worst:.3e}")


def test_constraint_rows_on_the_optimizer_variables_equal_the_row_by_row_mapping():
    from flobaroid_amd import excitation as exc

    rng = np.random.default_rng(2)
    n, nh, P = 4, 3, 6
    nf = [3, 2, 3, 1]
    lim = [(-1.0, 2.0), (-0.5, 0.5), (-2.0, 1.0), (-1.0, 1.0)]
    grad = {"wf": rng.standard_normal(P), "q_offset": rng.standard_normal((P, n)), "q_range": rng.standard_normal((P, n)),
            "a": rng.standard_normal((P, n, nh)), "b": rng.standard_normal((P, n, nh))}
    q0 = np.array([10.0, 40.0, -20.0, 0.0])
    for cand, kw in (({"q_range": None}, {}), ({"q_range": None}, {"use_deg": True}), ({"q_range": np.ones(n)}, {}),
                     ({"q_range": np.ones(n)}, {"use_deg": True, "exact": True, "joint_limits": lim, "q0": q0})):
        got = exc.constraint_gradient_to_optimizer_variables(grad, cand, nf, **kw)
        assert got.shape == (P, 1 + n + 2 * sum(nf))
        for k in range(P):
            row = exc.gradient_to_optimizer_variables({key: v[k] for key, v in grad.items()}, cand, nf, **kw)
            assert np.array_equal(got[k], row)


def test_gradient_symbols_and_version():
    """the two new entry points exist in the header, the binding and the library; the version is still 104"""
    from flobaroid_amd import _lib

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    for name in ("fbr_capsule_distance_gradients", "fbr_fourier_position_chain"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr), name
    assert lib.fbr_version() == _lib.FBR_VERSION == 104 == int(re.search(r"#define FBR_VERSION (\d+)", hdr).group(1))
    assert hasattr(_lib.Engine, "capsule_distance_gradients") and hasattr(_lib.Engine, "fourier_position_chain")
