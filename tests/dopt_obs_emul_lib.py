"""Loader of the CPU emulation of the eigenvector / observability text of csrc/fbr_dopt.h (tests/emul/dopt_obs_emul.cpp, g++
-ffp-contract=off; lanes run one after the other), as tests/dopt_emul_lib.py loads the terms."""
import ctypes
import os
import subprocess

import numpy as np

from dopt_emul_lib import ROOT, _dp, _ip

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "emul", "dopt_obs_emul.cpp")
_OUT = os.path.join(_HERE, "emul", "_build", "libdopt_obs_emul.so")
_DEPS = [SRC] + [os.path.join(ROOT, "flobaroid_amd", "csrc", h) for h in ("fbr_dopt.h", "fbr_math.h")] + [os.path.join(ROOT, "include", "fbr.h")]
_lib = None


def emul():
    global _lib
    if _lib is None:
        if not os.path.exists(_OUT) or any(os.path.getmtime(d) > os.path.getmtime(_OUT) for d in _DEPS):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", _OUT, SRC])
        _lib = ctypes.CDLL(_OUT)
        _lib.dopt_obs_emul_band.restype = ctypes.c_double
    return _lib


def band(n):
    return float(emul().dopt_obs_emul_band(int(n)))


def dopt_observability(G, cols, threshold=1e-6, prior=None, eigenvalues=True, vectors=True, nt=64):
    """the dict of Engine.dopt_observability (NumPy arrays) from the emulation; None where the device call refuses"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    C, Pa = G.shape[0], G.shape[1]
    ca = np.ascontiguousarray(cols, dtype=np.int32)
    n = ca.size
    pr = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
    nobs, status = np.zeros(C, dtype=np.int32), np.zeros(C, dtype=np.int32)
    energy, margin = np.empty((C, n)), np.empty(C)
    eig = np.empty((C, n)) if eigenvalues else None
    vec = np.empty((C, n, n)) if vectors else None
    d = lambda a: None if a is None else a.ctypes.data_as(_dp)  # noqa: E731
    rc = emul().dopt_obs_emul(d(G), C, Pa, ca.ctypes.data_as(_ip), n, d(pr), ctypes.c_double(threshold), int(nt), nobs.ctypes.data_as(_ip),
                              d(energy), d(margin), d(eig), d(vec), status.ctypes.data_as(_ip))
    if rc != 0:
        return None
    out = {"n_observable": nobs.astype(np.int64), "energy": energy, "margin": margin, "status": status}
    if eigenvalues:
        out["eig"] = eig
    if vectors:
        out["vec"] = vec
    return out
