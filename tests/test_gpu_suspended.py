"""fbr_suspended_base_motion / Engine.suspended_base_motion against the CPU restatement of the reference's loop
(tests/suspended_restatement.py, form (a): a full world-frame Newton-Euler at every step).

Bars are measured, not fixed: the yardstick is form (a) in np.longdouble, the bar of a quantity is 10 x the largest deviation the
double-precision form (a) itself shows against it on the same inputs, with a floor of 32 eps of the quantity's scale (a value that went
through a few dozen roundings cannot be asked to be closer than that).  Scales: 1 rad for angles, max |omega| for rates, max |value| of the
yardstick for positions and twists, max |base_vel| / dt for base_acc; a record field by max(max |I|, max |field|) (pose entries: 1).
Every figure is printed next to its bar."""
import numpy as np
import pytest

import suspended_restatement as sr
from common import load_topo, random_topology
from test_suspended_host import hanging_pose, prismatic_tree, smooth_states

pytestmark = pytest.mark.gpu
EPS = 2.0**-52
DT = 1 / 200.0

# name -> (robot, attachment, damping, amplitude, seed).  The smooth cases move about a pose that hangs nearly straight below the
# attachment (hanging_pose; WALK-MAN on crane_ft hangs that way by construction), so that no angle reaches the clamp; the clamp case
# swings a random pose at large amplitude under weak damping.
CASES = {
    "leftarm-LShy": ("walkman_left_arm", "LShy", 500.0, 0.15, 21),
    "leftarm-LSoftHandLink": ("walkman_left_arm", "LSoftHandLink", 500.0, 0.15, 22),
    "leftarm-Waist": ("walkman_left_arm", "Waist", 500.0, 0.05, 23),
    "walkman-crane_ft": ("walkman_apriori", "crane_ft", 2000.0, 0.3, 24),
    "prismatic": ("prismatic", None, 50.0, 0.15, 25),
    "leftarm-Waist-clamp": ("walkman_left_arm", "Waist", 5.0, 1.6, 3),
}
SHAPES = {"leftarm-LShy": [(3, 65), (65, 3), (1, 1), (2, 2)]}
_cache, _pose = {}, {}


def _setup(name):
    robot, att, damping, amp, seed = CASES[name]
    if robot == "prismatic":
        topo, al = prismatic_tree()
    else:
        topo = load_topo(robot)
        al = list(topo.link_names).index(att)
    return topo, al, damping, amp, seed


def _engine(topo, options=None):
    from flobaroid_amd._lib import Engine

    return Engine(topo, floating=True, options=options)


def _inputs(name, C, T):
    topo, al, damping, amp, seed = _setup(name)
    rng = np.random.default_rng(seed)
    if name not in _pose:
        _pose[name] = None if name.endswith("clamp") or name.startswith("walkman-") else hanging_pose(topo, al, np.random.default_rng(seed))
    q, dq, ddq = smooth_states(topo, C, T, rng, amp=amp, q0=_pose[name])
    return topo, al, damping, {"q": q, "dq": dq, "ddq": ddq}


def _reference(name, C, T):
    """(inputs, form (a) in double, form (a) in long double), computed once per case and shape"""
    key = (name, C, T)
    if key not in _cache:
        topo, al, damping, st = _inputs(name, C, T)
        a = sr.simulate_direct(topo, al, st["q"], st["dq"], st["ddq"], C, DT, damping)
        y = sr.simulate_direct(topo, al, st["q"], st["dq"], st["ddq"], C, DT, damping, dtype=np.longdouble)
        _cache[key] = (topo, al, damping, st, a, y)
    return _cache[key]


def _cuda(st):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in st.items()}


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _check(label, got, a, y, scale):
    scale = float(scale) if float(scale) > 0 else 1.0
    dev_a = float(np.abs(a.astype(np.longdouble) - y).max()) / scale
    dev_g = float(np.abs(got.astype(np.longdouble) - y).max()) / scale
    bar = max(10 * dev_a, 32 * EPS)
    print(f"  {label:24s} device {dev_g:.2e}   double (a) {dev_a:.2e}   bar {bar:.2e}")
    return dev_g <= bar, f"{label}: device {dev_g:.3e} > bar {bar:.3e} (double (a): {dev_a:.3e})"


def _motion_checks(name, C, T, got, a, y):
    wmax = float(np.abs(y["att_state"][:, 3:]).max())
    vmax = float(np.abs(y["base_vel"]).max())
    res = [
        _check("base_rpy", _host(got["rpy"]), a["rpy"], y["rpy"], 1.0),
        _check("base_pos", _host(got["base_position"]), a["base_position"], y["base_position"], np.abs(y["base_position"]).max()),
        _check("base_vel", _host(got["base_vel"]), a["base_vel"], y["base_vel"], vmax),
        _check("base_acc", _host(got["base_acc"]), a["base_acc"], y["base_acc"], vmax / DT),
        _check("att rpy", _host(got["att_state"])[:, :3], a["att_state"][:, :3], y["att_state"][:, :3], 1.0),
        _check("att omega", _host(got["att_state"])[:, 3:], a["att_state"][:, 3:], y["att_state"][:, 3:], wmax),
    ]
    bad = [msg for ok, msg in res if not ok]
    assert not bad, f"{name} C={C} T={T}: " + "; ".join(bad)


MOTION = [(n, C, T) for n in CASES for (C, T) in SHAPES.get(n, [(3, 65)])]


@pytest.mark.parametrize("name,C,T", MOTION, ids=[f"{n}-{C}x{T}" for n, C, T in MOTION])
def test_motion_parity(name, C, T):
    topo, al, damping, st, a, y = _reference(name, C, T)
    clamp = name.endswith("clamp")
    stats = a["stats"]
    if clamp:  # conditions on the restatement itself: the seed is chosen so that form (a) alone satisfies them
        assert stats["reversals"].sum() >= 1 and stats["free_after_clamp"].sum() >= 1 and stats["margin"] > 1e-9, stats
        assert np.array_equal(a["info"], y["info"])
    else:
        assert not a["info"][:, 1].any()
    if name.startswith("walkman"):
        assert (a["info"][:, 0] < sr.EQ_MAX_ITER).all()
    eng = _engine(topo)
    got = eng.suspended_base_motion(_cuda(st), C, topo.x_std(), al, DT, damping, with_info=True)
    print(f"{name} C={C} T={T}: iterations {a['info'][:, 0].tolist()[:4]}, clamp events {a['info'][:, 1].tolist()[:4]}")
    assert np.array_equal(_host(got["info"]), a["info"])
    _motion_checks(name, C, T, got, a, y)
    if T <= 2:
        assert not _host(got["base_acc"]).any()


RECORD_CASES = [n for n in CASES if not n.endswith("clamp")]


@pytest.mark.parametrize("name", RECORD_CASES)
def test_record_parity(name):
    """kernel 1 alone: every entry of the 195 records (four blocks, the last with three live lanes)"""
    C, T = 3, 65
    topo, al, damping, st = _inputs(name, C, T)
    a = sr.sample_records(topo, al, st["q"], st["dq"], st["ddq"])
    y = sr.sample_records(topo, al, st["q"], st["dq"], st["ddq"], dtype=np.longdouble)
    eng = _engine(topo)
    got = _host(eng.suspended_records(_cuda(st), topo.x_std(), al))
    assert got.shape == (C * T, sr.REC)
    imax = float(np.abs(y[:, :6]).max())
    fields = {"I": (0, 6, imax), "B": (6, 15, None), "c0": (15, 18, None), "mc": (18, 21, None), "pose R": (21, 30, 1.0), "pose p": (30, 33, 1.0),
              "twist": (33, 39, 0.0)}
    bad = []
    print(f"{name}: max |I| {imax:.3g}")
    for label, (i0, i1, scale) in fields.items():
        fmax = float(np.abs(y[:, i0:i1]).max())
        scale = max(imax, fmax) if scale is None else max(scale, fmax)
        ok, msg = _check(label, got[:, i0:i1], a[:, i0:i1], y[:, i0:i1], scale)
        if not ok:
            bad.append(msg)
    assert not bad, f"{name}: " + "; ".join(bad)


def test_independence_and_determinism():
    """candidate c of a batch equals the single-candidate call on it; two runs, host / device outputs and host / device inputs: same bits"""
    name, C, T = "leftarm-LShy", 3, 65
    topo, al, damping, st = _inputs(name, C, T)
    eng = _engine(topo)
    x = topo.x_std()
    dev = _cuda(st)
    keys = ("rpy", "base_position", "base_vel", "base_acc", "att_state", "info")
    full = {k: _host(v) for k, v in eng.suspended_base_motion(dev, C, x, al, DT, damping, with_info=True).items()}
    again = eng.suspended_base_motion(dev, C, x, al, DT, damping, with_info=True)
    to_host = eng.suspended_base_motion(dev, C, x, al, DT, damping, device_out=False, with_info=True)
    from_host = eng.suspended_base_motion(st, C, x, al, DT, damping, with_info=True)
    for k in keys:
        assert isinstance(to_host[k], np.ndarray) and isinstance(from_host[k], np.ndarray)
        for other in (again, to_host, from_host):
            assert np.array_equal(full[k], _host(other[k])), k
    plain = eng.suspended_base_motion(dev, C, x, al, DT, damping)
    assert set(plain) == {"rpy", "base_position", "base_vel", "base_acc"} and all(np.array_equal(full[k], _host(plain[k])) for k in plain)
    for c in range(C):
        one = eng.suspended_base_motion({k: v[c * T:(c + 1) * T] for k, v in dev.items()}, 1, x, al, DT, damping, with_info=True)
        for k in keys:
            ref = full[k][c:c + 1] if k == "info" else full[k][c * T:(c + 1) * T]
            assert np.array_equal(ref, _host(one[k])), (c, k)


def test_nan_inputs_end():
    """NaN inputs give NaN outputs and the loops end (their bounds are T and 200)"""
    topo, al, damping, st = _inputs("leftarm-LShy", 2, 5)
    st = {k: v.copy() for k, v in st.items()}
    st["q"][:5] = np.nan
    eng = _engine(topo)
    got = eng.suspended_base_motion(st, 2, topo.x_std(), al, DT, damping, with_info=True)
    assert np.isnan(got["rpy"][:5]).all() and np.isfinite(got["rpy"][5:]).all()
    assert got["info"][0, 0] == sr.EQ_MAX_ITER


def test_errors_and_limits():
    from flobaroid_amd._lib import Engine, FbrError

    topo, al, damping, st = _inputs("leftarm-LShy", 3, 4)
    x = topo.x_std()
    eng = _engine(topo)
    ok = lambda e=eng: e.suspended_base_motion(st, 3, x, al, DT, damping)  # noqa: E731
    ok()
    bad = [
        lambda: eng.suspended_base_motion(st, 3, x, -1, DT, damping),
        lambda: eng.suspended_base_motion(st, 3, x, topo.num_links, DT, damping),
        lambda: eng.suspended_base_motion(st, 3, x, al, 0.0, damping),
        lambda: eng.suspended_base_motion(st, 3, x, al, -DT, damping),
        lambda: eng.suspended_base_motion(st, 3, x, al, float("nan"), damping),
        lambda: eng.suspended_base_motion(st, 3, x, al, float("inf"), damping),
        lambda: eng.suspended_base_motion(st, 3, x, al, DT, -1.0),
        lambda: eng.suspended_base_motion(st, 3, x, al, DT, float("nan")),
        lambda: eng.suspended_base_motion(st, 0, x, al, DT, damping),
        lambda: eng.suspended_base_motion(st, 5, x, al, DT, damping),
        lambda: eng.suspended_base_motion({k: v[:0] for k, v in st.items()}, 1, x, al, DT, damping),
        lambda: eng.suspended_base_motion(st, 3, x[: 10 * topo.num_links - 1], al, DT, damping),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(FbrError, match=r"code -1\b"):
            f()
        ok()  # the handle stays usable
    fixed = Engine(topo, floating=False)
    with pytest.raises(FbrError, match=r"code -1\b.*floating"):
        fixed.suspended_base_motion(st, 3, x, al, DT, damping)
    eng.set_option("fused_id", 0)
    with pytest.raises(FbrError, match=r"code -4\b.*fused_id"):
        ok()
    eng.set_option("fused_id", 1)
    ok()
    chain = random_topology(np.random.default_rng(1), 26, p_fixed=0.0, branchiness=0.0)
    assert chain.num_dofs == 25
    deep = Engine(chain, floating=True)
    z = np.zeros((2, 25))
    with pytest.raises(FbrError, match=r"code -4\b.*24 joints"):
        deep.suspended_base_motion({"q": z, "dq": z, "ddq": z}, 1, chain.x_std(), 25, DT, damping)
    deep.inverse_dynamics({"q": z, "dq": z, "ddq": z, "base_vel": np.zeros((2, 6)), "base_acc": np.zeros((2, 6)), "rpy": np.zeros((2, 3))}, chain.x_std())


def test_abi():
    import ctypes
    import os
    import re

    from common import ROOT
    from flobaroid_amd import _lib

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    assert hasattr(lib, "fbr_suspended_base_motion") and re.search(r"\bint fbr_suspended_base_motion\(", hdr)
    assert isinstance(lib.fbr_suspended_base_motion, ctypes._CFuncPtr)
    assert lib.fbr_version() == 104
