"""Loader of the CPU emulation of csrc/fbr_dopt.h (tests/emul/dopt_emul.cpp, g++ -ffp-contract=off; lanes run one after the other)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
SRC = os.path.join(_HERE, "emul", "dopt_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libdopt_emul.so")
_DEPS = [SRC] + [os.path.join(ROOT, "flobaroid_amd", "csrc", h) for h in ("fbr_dopt.h", "fbr_math.h")] + [os.path.join(ROOT, "include", "fbr.h")]
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lib = None


def emul():
    global _lib
    if _lib is None:
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in _DEPS):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, SRC])
        _lib = ctypes.CDLL(_OUT)
    return _lib


def dopt_terms(G, cols, reg=1e-4, prior=None, scale=None, eigenvalues=True, weights=True, nt=64):
    """the dict of Engine.dopt_terms (NumPy arrays) from the emulation; a non-zero status does not raise"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    C, Pa = G.shape[0], G.shape[1]
    ca = np.ascontiguousarray(cols, dtype=np.int32)
    n = ca.size
    pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
    sc = None if scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (C,)))
    terms, status = np.empty((C, 4)), np.zeros(C, dtype=np.int32)
    eig = np.empty((C, n)) if eigenvalues else None
    Cm = np.empty((C, n, n)) if weights else None
    d = lambda a: None if a is None else a.ctypes.data_as(_dp)  # noqa: E731
    rc = emul().dopt_emul(d(G), C, Pa, ca.ctypes.data_as(_ip), n, d(pr), ctypes.c_double(reg), d(sc), int(nt), d(terms),
                          status.ctypes.data_as(_ip), d(eig), d(Cm))
    assert rc == 0
    out = {"neg_log_det": terms[:, 0].copy(), "lambda_max": terms[:, 1].copy(), "delta": terms[:, 2].copy(),
           "n_observable": terms[:, 3].astype(np.int64), "status": status}
    if eigenvalues:
        out["eig"] = eig
    if weights:
        out["Cmat"] = Cm
    return out
