"""The producer's wave-wide sum of a column group's rhs moments (csrc/fbr_mom_lanes.h: fbr_mom_lanes_sum), without a GPU.

tests/emul/gram64_mom_lanes.cpp runs the template the device runs on 64 emulated lanes.  Here: for groups of 1, 2, 3, 4 and 6 columns
and every number of live lanes, the lanes of a column's class hold exactly the sum that the documented order gives (restated below,
independently of the template), that sum is as good as a tree of depth six must be, the dead lanes -- which hold NaN -- do not get
through, and the lanes that add a link's ten parameters are ten different ones inside the right classes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "gram64_mom_lanes.cpp")
_HDR = os.path.join(_HERE, "..", "flobaroid_amd", "csrc", "fbr_mom_lanes.h")
_OUT = os.path.join(_HERE, "emul", "_build", "libgram64_mom_lanes.so")
_lib = None
_dp = ctypes.POINTER(ctypes.c_double)


def lib():
    global _lib
    if _lib is None:
        deps = [_SRC, _HDR, os.path.join(os.path.dirname(_HDR), "fbr_math.h")]
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in deps):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            tmp = f"{_OUT}.{os.getpid()}"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, _SRC])
            os.replace(tmp, _OUT)
        _lib = ctypes.CDLL(_OUT)
    return _lib


def lanes_sum(v, valid):
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.full(64, np.nan)
    assert lib().mom_lanes_sum(v.shape[0], v.ctypes.data_as(_dp), int(valid), out.ctypes.data_as(_dp)) == 0
    return out


# the lanes that hold column c of a group of nq afterwards: the halves split the columns first, the rows of 16 lanes second, bit 8 of the
# lane tells the two values apart that a group of six has left in a row
CLASSES = {
    1: {0: range(64)},
    2: {0: range(0, 32), 1: range(32, 64)},
    3: {0: range(0, 16), 1: range(16, 32), 2: range(32, 48)},
    4: {0: range(0, 16), 1: range(16, 32), 2: range(32, 48), 3: range(48, 64)},
    6: {0: range(0, 8), 1: range(8, 16), 2: range(16, 24), 3: range(32, 40), 4: range(40, 48), 5: range(48, 56)},
}


def documented_sum(x):
    """the order of fbr_mom_lanes.h on the 64 lanes' values x (dead lanes already zero), in float64"""
    a = [np.float64(x[i]) + np.float64(x[i + 32]) for i in range(32)]
    b = [a[i] + a[i + 16] for i in range(16)]
    for mask in (8, 7, 2, 1):
        b = [b[i] + b[i ^ mask] for i in range(16)]
    assert all(v == b[0] for v in b)  # (every lane of the row ends with the same bits)
    return b[0]


def test_classes_cover_what_the_header_says():
    for nq, cls in CLASSES.items():
        got = [lib().mom_lanes_class(nq, lane) for lane in range(64)]
        want = [-1] * 64
        for c, lanes in cls.items():
            for lane in lanes:
                want[lane] = c
        assert got == want, nq


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 6])
def test_sum_in_the_documented_order(nq):
    rng = np.random.default_rng(700 + nq)
    for valid in range(1, 65):
        v = rng.standard_normal((nq, 64)) * 10.0 ** rng.integers(-3, 4, (nq, 64))  # (mixed magnitudes: the order shows)
        v[:, valid:] = np.nan
        out = lanes_sum(v, valid)
        # what is in the dead lanes does not matter
        v2 = v.copy()
        v2[:, valid:] = np.inf
        assert np.array_equal(out, lanes_sum(v2, valid))
        held = np.zeros(64, dtype=bool)
        for c, lanes in CLASSES[nq].items():
            x = np.where(np.arange(64) < valid, v[c], 0.0)
            want = documented_sum(x)
            assert np.array_equal(out[list(lanes)], np.full(len(lanes), want)), (nq, valid, c)
            ref = sum((np.longdouble(t) for t in x), np.longdouble(0))
            assert abs(np.longdouble(want) - ref) <= 64 * 2.0 ** -53 * np.abs(x).sum(), (nq, valid, c)
            held[list(lanes)] = True
        assert np.array_equal(out[~held], np.zeros(int((~held).sum())))  # (the other lanes: sums of zeros, never a dead lane's NaN)


def test_one_live_lane_keeps_its_value_to_the_bit():
    v = np.full((4, 64), np.nan)
    v[:, 0] = [1.0 / 3.0, -2.0 / 7.0, 1e-300, 1e300]
    out = lanes_sum(v, 1)
    for c in range(4):
        assert np.array_equal(out[16 * c: 16 * c + 16], np.full(16, v[c, 0]))


def test_parameter_lanes():
    """twenty parameter lanes (ten per rhs column) and eight friction lanes: all different, each parameter's inside the class of its
    column -- parameters 0 .. 3 are summed as a group of four, 4 .. 9 as a group of six"""
    lanes = {(p, r): lib().mom_lane(p, r) for r in (0, 1) for p in range(10)}
    fric = {(pf, r): lib().mom_fric_lane(pf, r) for r in (0, 1) for pf in range(4)}
    assert len(set(lanes[p, 0] for p in range(10))) == 10  # injective on 0 .. 9
    every = list(lanes.values()) + list(fric.values())
    assert len(set(every)) == 28 and all(0 <= x < 64 for x in every)
    for (p, r), lane in lanes.items():
        assert lane in (CLASSES[4][p] if p < 4 else CLASSES[6][p - 4]), (p, r)
