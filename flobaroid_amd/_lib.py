"""Thin ctypes layer over the C-ABI in ``include/fbr.h`` (``libfbr.so``, HIP, gfx950).

There is no CPU fallback: if the shared library is missing or no HIP device is usable the calls
raise.  Arrays may be NumPy (host) or torch CUDA tensors (device, float64, contiguous); all state
arrays of one call must live in the same memory space.
"""
from __future__ import annotations

import ctypes
import os
from typing import Any

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FBR_LIB_PATH") or os.path.join(_HERE, "libfbr.so")  # (FBR_LIB_PATH: kernel-shape experiments, tools/)

FBR_HOST = 0
FBR_DEVICE = 1

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


class FbrError(RuntimeError):
    pass


class fbr_topology(ctypes.Structure):
    _fields_ = [
        ("num_links", ctypes.c_int32),
        ("num_dofs", ctypes.c_int32),
        ("parent", _ip),
        ("dof_index", _ip),
        ("rest_R", _dp),
        ("rest_p", _dp),
        ("axis", _dp),
        ("floating_base", ctypes.c_int32),
        ("gravity", ctypes.c_double * 3),
        ("friction", ctypes.c_int32),
        ("friction_symmetric", ctypes.c_int32),
        ("gravity_only", ctypes.c_int32),
        ("stribeck_velocity", ctypes.c_double),
        ("joint_type", _ip),
    ]


class fbr_states(ctypes.Structure):
    _fields_ = [
        ("num_samples", ctypes.c_int64),
        ("mem", ctypes.c_int32),
        ("q", ctypes.c_void_p),
        ("dq", ctypes.c_void_p),
        ("ddq", ctypes.c_void_p),
        ("base_vel", ctypes.c_void_p),
        ("base_acc", ctypes.c_void_p),
        ("base_rpy", ctypes.c_void_p),
        ("sign", ctypes.c_void_p),
    ]


_lib = None

# name -> (restype, argtypes); also the list of symbols tests check against include/fbr.h
_SIGNATURES = {
    "fbr_version": (ctypes.c_int, []),
    "fbr_device_count": (ctypes.c_int, []),
    "fbr_last_error": (ctypes.c_char_p, []),
    "fbr_model_create": (ctypes.c_int, [ctypes.POINTER(fbr_topology), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "fbr_model_destroy": (None, [ctypes.c_void_p]),
    "fbr_model_dims": (ctypes.c_int, [ctypes.c_void_p, _ip, _ip]),
    "fbr_model_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "fbr_regressor_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32]),
    "fbr_inverse_dynamics_batch": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), _dp, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_candidate_extrema": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_int32, _dp, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_int32],
    ),
    "fbr_torque_row_sweep": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, _dp, ctypes.c_int32,
         ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_suspended_base_motion": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_int32, _dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_suspended_records": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), _dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_model_set_capsules": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _ip, _dp, _dp, ctypes.c_int32, _ip]),
    "fbr_candidate_capsule_distances": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_int32],
    ),
    "fbr_capsule_distance_gradients": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_model_set_boxes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _ip, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_int32, _ip]),
    "fbr_candidate_box_distances": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_int32],
    ),
    "fbr_model_set_hulls": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _ip, _dp, _dp, ctypes.c_int32, _ip, _dp, _ip, _dp, _ip, _ip, ctypes.c_int32,
                                           _ip]),
    "fbr_model_set_large_hulls": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _ip, _dp, _dp, ctypes.c_int32, _ip, _dp, _ip, _dp, _ip, _ip,
                                                 ctypes.c_int32, _ip]),
    "fbr_model_set_hull_meshes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _ip, _ip, _dp]),
    "fbr_model_set_large_hull_meshes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _ip, _ip, _dp]),
    "fbr_candidate_hull_distances": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_int32],
    ),
    "fbr_box_distance_gradients": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_hull_distance_gradients": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_mesh_distance_gradients": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_large_hull_distance_gradients": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_large_mesh_distance_gradients": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_predict": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(fbr_states), _dp, ctypes.c_void_p, ctypes.c_int32]),
    "fbr_contact_torques": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_int32, _dp, _dp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_gram_accumulate": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_int32, ctypes.c_int32],
    ),
    "fbr_gram_submit": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)],
    ),
    "fbr_wait": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "fbr_gram_grouped": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_int32],
    ),
    "fbr_fd_scores": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_fourier_states": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, _dp, _dp, _dp, _dp, _dp, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_regressor_weights": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_int32, _ip, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_dopt_terms": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, _ip, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double, _dp,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_dopt_observability": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, _ip, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_fourier_gradient": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, _dp, _dp, _dp, _dp, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_fourier_position_chain": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, _dp, _dp, _dp, _dp, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_fourier_state_chain": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, _dp, _dp, _dp, _dp, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_tsqr": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_tsqr_cols": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), _ip, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32],
    ),
    "fbr_tsqr_submit": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(fbr_states), _ip, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)],
    ),
    "fbr_tsqr_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]),
    "fbr_tsqr_work_info": (
        ctypes.c_int,
        [ctypes.c_void_p, _ip, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
         ctypes.POINTER(ctypes.c_int64), _ip, _ip],
    ),
    "fbr_filtfilt": (ctypes.c_int, [ctypes.c_void_p, _dp, _dp, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "fbr_medfilt": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "fbr_central_diff": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "fbr_profile_enable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "fbr_profile_get": (ctypes.c_int, [ctypes.c_void_p, _dp, ctypes.POINTER(ctypes.c_int64)]),
    "fbr_gram_program_info": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, _ip, _ip, ctypes.POINTER(ctypes.c_int64), _ip],
    ),
    "fbr_gram_lane_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "fbr_model_link_merge_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, _ip, _ip]),
    "fbr_model_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double]),
    "fbr_model_get_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double)]),
    "fbr_model_option_name": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.c_char_p)]),
}

# Options every new Engine starts with (``fbr_model_set_option``, include/fbr.h lists the keys), on top of the library's defaults and below
# the ``options`` argument of the constructor.  A plain Python dict: the library itself never reads the process environment.  The test
# suite uses it to run whole modules with the column reductions forced / switched off (tests/conftest.py: reduction_mode).
FBR_VERSION = 104  # include/fbr.h FBR_VERSION: the C-ABI these ctypes signatures describe
FBR_MAX_HULL_VERTICES = 128  # include/fbr.h: a hull of Engine.set_hulls
FBR_MAX_LARGE_HULL_VERTICES = 1024  # include/fbr.h: a hull of Engine.set_hulls(..., large=True)
FBR_MAX_LARGE_MESH_TRIANGLES = 8192  # include/fbr.h: a mesh of Engine.set_large_hull_meshes / set_hulls(..., large_meshes=True)
FBR_MAX_DOPT_COLUMNS = 512  # include/fbr.h: the selected columns of Engine.dopt_terms
DEFAULT_OPTIONS: dict = {}


def load_library():
    """Load libfbr.so (fails loudly; never substitutes a CPU path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FbrError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  flobaroid_amd has no CPU fallback."
        )
    # torch ships its own libamdhip64; if libfbr pulled in /opt/rocm's copy first, a later torch.cuda
    # initialisation in the same process would see "No HIP GPUs".  Load torch's runtime first when torch
    # is installed so both share one HIP runtime (torch is plumbing here, not a dependency of the C-ABI).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    missing = [name for name in _SIGNATURES if not hasattr(lib, name)]
    if missing:  # (entry points have been added without a new FBR_VERSION: an older library of the same number lacks them)
        raise FbrError(f"{LIB_PATH} does not export {', '.join(missing)}: it was built from older sources -- rebuild it with "
                       "`python -c 'import __graft_entry__ as g; g.build()'`")
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    got = int(lib.fbr_version())
    if got != FBR_VERSION:
        raise FbrError(f"{LIB_PATH} reports C-ABI version {got}, this binding was written for {FBR_VERSION} (include/fbr.h FBR_VERSION): "
                       "rebuild it with `python -c 'import __graft_entry__ as g; g.build()'` -- signatures have changed between the two")
    _lib = lib
    return lib


def device_count() -> int:
    return int(load_library().fbr_device_count())


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_library().fbr_last_error()
        raise FbrError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def _is_torch(x: Any) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


class _Ref:
    """Pointer + memory space of one array argument (keeps the backing object alive)."""

    def __init__(self, x: Any, shape: tuple | None = None, name: str = "array"):
        self.obj = None
        self.ptr = None
        self.mem = None
        if x is None:
            return
        if _is_torch(x):
            import torch

            if x.dtype != torch.float64:
                raise TypeError(f"{name}: torch tensors must be float64")
            if x.device.type == "cuda":
                t = x.contiguous()
                self.obj, self.ptr, self.mem = t, t.data_ptr(), FBR_DEVICE
                got = tuple(t.shape)
            else:
                a = np.ascontiguousarray(x.numpy(), dtype=np.float64)
                self.obj, self.ptr, self.mem = a, a.ctypes.data, FBR_HOST
                got = a.shape
        else:
            a = np.ascontiguousarray(x, dtype=np.float64)
            self.obj, self.ptr, self.mem = a, a.ctypes.data, FBR_HOST
            got = a.shape
        if shape is not None and tuple(got) != tuple(shape):
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(got)}")


def _same_space(refs: list[_Ref]) -> int:
    mems = {r.mem for r in refs if r.mem is not None}
    if len(mems) > 1:
        raise ValueError("all arrays of one call must live in the same memory space (all NumPy or all CUDA tensors)")
    return mems.pop() if mems else FBR_HOST


class Engine:
    """One ``fbr_model`` handle: device tables of a robot + identified-column layout."""

    def __init__(self, topo, floating=False, friction=False, friction_symmetric=True, gravity_only=False,
                 stribeck_velocity=0.0, gravity=(0.0, 0.0, -9.81), device: int = 0, options: dict | None = None):
        lib = load_library()
        self._lib = lib
        self.topo = topo
        self._parent = np.array(topo.parent, dtype=np.int32)
        self._dof = np.array(topo.dof_index, dtype=np.int32)
        self._restR = np.ascontiguousarray(topo.rest_R, dtype=np.float64).reshape(-1)
        self._restp = np.ascontiguousarray(topo.rest_p, dtype=np.float64).reshape(-1)
        self._axis = np.ascontiguousarray(topo.axis, dtype=np.float64).reshape(-1)
        t = fbr_topology()
        t.num_links = topo.num_links
        t.num_dofs = topo.num_dofs
        t.parent = self._parent.ctypes.data_as(_ip)
        t.dof_index = self._dof.ctypes.data_as(_ip)
        t.rest_R = self._restR.ctypes.data_as(_dp)
        t.rest_p = self._restp.ctypes.data_as(_dp)
        t.axis = self._axis.ctypes.data_as(_dp)
        t.floating_base = int(bool(floating))
        t.gravity = (ctypes.c_double * 3)(*[float(g) for g in gravity])
        t.friction = int(bool(friction))
        t.friction_symmetric = int(bool(friction_symmetric))
        t.gravity_only = int(bool(gravity_only))
        t.stribeck_velocity = float(stribeck_velocity)
        self._jtype = np.array(topo.joint_type, dtype=np.int32)  # 0 fixed, 1 revolute, 2 prismatic
        t.joint_type = self._jtype.ctypes.data_as(_ip)
        h = ctypes.c_void_p()
        _check(lib.fbr_model_create(ctypes.byref(t), int(device), ctypes.byref(h)), "fbr_model_create")
        self._h = h
        r, c = ctypes.c_int32(), ctypes.c_int32()
        _check(lib.fbr_model_dims(h, ctypes.byref(r), ctypes.byref(c)), "fbr_model_dims")
        self.rows, self.cols = int(r.value), int(c.value)
        self.n = topo.num_dofs
        self.L = topo.num_links
        self.floating = bool(floating)
        self.friction = bool(friction)
        self.stribeck = float(stribeck_velocity) if friction else 0.0  # > 0: the torques need vel_sign
        self.device = int(device)
        for key, val in {**DEFAULT_OPTIONS, **(options or {})}.items():
            self.set_option(key, val)

    # ------------------------------------------------------------------ options (fbr_model_set_option)
    def set_option(self, key: str, value: float) -> None:
        _check(self._lib.fbr_model_set_option(self._h, key.encode(), float(value)), f"fbr_model_set_option({key})")

    def get_option(self, key: str) -> float:
        v = ctypes.c_double()
        _check(self._lib.fbr_model_get_option(self._h, key.encode(), ctypes.byref(v)), f"fbr_model_get_option({key})")
        return float(v.value)

    def options(self) -> dict:
        """Every option of the handle with its current value."""
        out, i, name = {}, 0, ctypes.c_char_p()
        while self._lib.fbr_model_option_name(i, ctypes.byref(name)) == 0:
            out[name.value.decode()] = self.get_option(name.value.decode())
            i += 1
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.fbr_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def set_stream(self, stream_ptr: int | None) -> None:
        _check(self._lib.fbr_model_set_stream(self._h, ctypes.c_void_p(stream_ptr or 0)), "fbr_model_set_stream")
        self._stream_handle = int(stream_ptr or 0)  # 0: the model's own stream

    def use_torch_stream(self) -> None:
        """Run on torch's current stream when that is a real stream object.  torch's DEFAULT stream is the null stream (handle 0),
        which the C-ABI reads as "the model's own stream": the engine then keeps its own non-blocking stream and every call with
        CUDA tensors first waits for torch's stream (``_sync_torch``), so inputs produced by torch kernels are complete."""
        import torch

        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def _sync_torch(self) -> None:
        # calls are blocking and the library synchronises its own stream on return; what is missing is the other direction:
        # torch kernels still writing the inputs on a stream the library does not run on.  Checked at EVERY call: the caller may have
        # switched torch streams (or called set_stream) since use_torch_stream().
        import torch

        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream == 0 or cur.cuda_stream != getattr(self, "_stream_handle", 0):
            cur.synchronize()

    def _states(self, st: dict, need_vel: bool = True):
        q = _Ref(st["q"], name="q")
        S = q.obj.shape[0]
        n = self.n
        if tuple(q.obj.shape) != (S, n):
            raise ValueError(f"q: expected (S,{n}), got {tuple(q.obj.shape)}")
        refs = [q]
        dq = _Ref(st.get("dq"), (S, n), "dq") if need_vel or st.get("dq") is not None else _Ref(None)
        ddq = _Ref(st.get("ddq"), (S, n), "ddq") if need_vel or st.get("ddq") is not None else _Ref(None)
        bv = ba = rpy = sg = _Ref(None)
        if self.floating:
            rpy = _Ref(st.get("rpy", st.get("base_rpy")), (S, 3), "base_rpy")
            if need_vel:
                bv = _Ref(st.get("base_vel", st.get("base_velocity")), (S, 6), "base_vel")
                ba = _Ref(st.get("base_acc", st.get("base_acceleration")), (S, 6), "base_acc")
        if self.friction and need_vel:
            sg = _Ref(st.get("sign"), (S, n), "sign")
        refs += [dq, ddq, bv, ba, rpy, sg]
        mem = _same_space(refs)
        if mem == FBR_DEVICE:
            self._sync_torch()
        s = fbr_states()
        s.num_samples = S
        s.mem = mem
        s.q, s.dq, s.ddq = q.ptr, dq.ptr, ddq.ptr
        s.base_vel, s.base_acc, s.base_rpy, s.sign = bv.ptr, ba.ptr, rpy.ptr, sg.ptr
        return s, refs, S, mem

    def _out(self, out, shape, mem):
        if out is not None:
            if _is_torch(out):
                import torch

                if out.dtype != torch.float64 or not out.is_contiguous():
                    raise ValueError("out must be a contiguous float64 tensor")
            elif not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.dtype == np.float64):
                raise ValueError("out must be a C-contiguous float64 ndarray")
            return _Ref(out, shape, "out"), out
        if mem == FBR_DEVICE:
            import torch

            t = torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.device}")
            return _Ref(t), t
        a = np.empty(shape, dtype=np.float64)
        return _Ref(a), a

    # ------------------------------------------------------------------ C-ABI calls
    def regressor(self, st: dict, out=None):
        """Stacked standard regressor (S*rows, cols)."""
        s, keep, S, mem = self._states(st)
        r, ret = self._out(out, (S * self.rows, self.cols), mem)
        _check(self._lib.fbr_regressor_batch(self._h, ctypes.byref(s), r.ptr, r.mem), "fbr_regressor_batch")
        return ret

    def inverse_dynamics(self, st: dict, x_std, vel_sign=None, out=None):
        s, keep, S, mem = self._states(st)
        x = np.ascontiguousarray(x_std, dtype=np.float64)
        vs = _Ref(vel_sign, (S, self.n), "vel_sign") if vel_sign is not None else _Ref(None)
        if vs.mem is not None and vs.mem != mem:
            raise ValueError("vel_sign must live in the same memory space as the states")
        r, ret = self._out(out, (S, self.rows), mem)
        _check(
            self._lib.fbr_inverse_dynamics_batch(self._h, ctypes.byref(s), x.ctypes.data_as(_dp), int(x.size), vs.ptr,
                                                 r.ptr, r.mem),
            "fbr_inverse_dynamics_batch",
        )
        return ret

    EXTREMA = ("q_min", "q_max", "dq_absmax", "tau_absmax")

    def candidate_extrema(self, st: dict, ncand: int, x_std, vel_sign=None, device_out: bool | None = None) -> dict:
        """Per-candidate extrema of ``ncand`` equal candidates stacked along the sample axis (``fbr_candidate_extrema``): a dict of (C, n)
        arrays -- values ``q_min``, ``q_max``, ``dq_absmax``, ``tau_absmax`` (joint rows of the torques ``inverse_dynamics`` returns, NaN
        counted as 0, inf as DBL_MAX) and their int64 sample indices inside the candidate, ``<name>_idx``.  Torch tensors when the states
        are on the device, NumPy arrays otherwise (``device_out`` overrides)."""
        s, keep, S, mem = self._states(st)
        x = np.ascontiguousarray(x_std, dtype=np.float64)
        vs = _Ref(vel_sign, (S, self.n), "vel_sign") if vel_sign is not None else _Ref(None)
        if vs.mem is not None and vs.mem != mem:
            raise ValueError("vel_sign must live in the same memory space as the states")
        C = int(ncand)
        shape = (max(C, 1), 4, self.n)  # (ncand < 1 is refused by the library)
        out_mem = mem if device_out is None else (FBR_DEVICE if device_out else FBR_HOST)
        if out_mem == FBR_DEVICE:
            import torch

            val = torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.device}")
            idx = torch.empty(shape, dtype=torch.int64, device=f"cuda:{self.device}")
            pv, pi = val.data_ptr(), idx.data_ptr()
        else:
            val, idx = np.empty(shape), np.empty(shape, dtype=np.int64)
            pv, pi = val.ctypes.data, idx.ctypes.data
        _check(
            self._lib.fbr_candidate_extrema(self._h, ctypes.byref(s), C, x.ctypes.data_as(_dp), int(x.size), vs.ptr, pv, pi, out_mem),
            "fbr_candidate_extrema",
        )
        out = {}
        for k, name in enumerate(self.EXTREMA):
            out[name] = val[:, k]
            out[name + "_idx"] = idx[:, k]
        return out

    def torque_row_sweep(self, st: dict, ncand: int, sample, x_std, eps: float, joint=None, vel_sign=None, device_out: bool | None = None):
        """Joint torque rows of chosen samples under the finite-difference sweep (``fbr_torque_row_sweep``): a (C, R, 1 + 3 n) array whose
        entry ``[c, r, 0]`` is torque row ``joint[c, r]`` of ``inverse_dynamics`` at sample ``sample[c, r]`` of candidate c and entry
        ``[c, r, 1 + kind * n + d]`` the same row with +eps on q_d / dq_d / ddq_d (the entry order of ``fd_scores``); the sign series,
        ``vel_sign`` and the base state stay the sample's own.  ``sample`` (C, R) int, 0 .. T - 1; ``joint`` (C, R) int, 0 .. n - 1, or None:
        R = n and row r is joint r.  An index out of range raises ``FbrError``.  A CUDA tensor when the states are on the device
        (``device_out`` overrides), else NumPy; the index arrays are brought to the memory space of the states."""
        s, keep, S, mem = self._states(st)
        x = np.ascontiguousarray(x_std, dtype=np.float64)
        vs = _Ref(vel_sign, (S, self.n), "vel_sign") if vel_sign is not None else _Ref(None)
        if vs.mem is not None and vs.mem != mem:
            raise ValueError("vel_sign must live in the same memory space as the states")
        C = int(ncand)
        shp = tuple(sample.shape)
        if len(shp) != 2 or shp[0] != max(C, 1):
            raise ValueError(f"sample: expected ({C}, R), got {shp}")
        R = int(shp[1])
        smp, psmp = self._index_array(sample, shp, mem, "sample")
        jnt, pjnt = (None, None) if joint is None else self._index_array(joint, shp, mem, "joint", dtype=np.int32)
        out_mem = mem if device_out is None else (FBR_DEVICE if device_out else FBR_HOST)
        r, ret = self._out(None, shp + (1 + 3 * self.n,), out_mem)
        _check(self._lib.fbr_torque_row_sweep(self._h, ctypes.byref(s), C, R, psmp, pjnt, x.ctypes.data_as(_dp), int(x.size), vs.ptr, float(eps),
                                              r.ptr, out_mem), "fbr_torque_row_sweep")
        return ret

    def _joint_states(self, st: dict):
        """q, dq, ddq of ``st`` alone as an ``fbr_states`` (the base arrays stay NULL): (struct, keep-alive refs, S, memory space)"""
        q = _Ref(st["q"], None, "q")
        if len(q.obj.shape) != 2 or q.obj.shape[1] != self.n:
            raise ValueError(f"q: expected (S, {self.n}), got {tuple(q.obj.shape)}")
        S = int(q.obj.shape[0])
        dq, ddq = _Ref(st["dq"], (S, self.n), "dq"), _Ref(st["ddq"], (S, self.n), "ddq")
        mem = _same_space([q, dq, ddq])
        if mem == FBR_DEVICE:
            self._sync_torch()
        s = fbr_states()
        s.num_samples, s.mem, s.q, s.dq, s.ddq = S, mem, q.ptr, dq.ptr, ddq.ptr
        return s, [q, dq, ddq], S, mem

    def _link_index(self, link) -> int:
        return list(self.topo.link_names).index(link) if isinstance(link, str) else int(link)

    def suspended_base_motion(self, st: dict, ncand: int, x_std, att_link, dt: float, damping: float, device_out: bool | None = None,
                              with_info: bool = False) -> dict:
        """Base motion of ``ncand`` equal candidates stacked in ``st`` (``q``, ``dq``, ``ddq``) of a robot hanging from a ball joint at the
        origin of ``att_link`` (a link index or name) -- ``fbr_suspended_base_motion``, the reference's ``simulate_suspended_base_motion`` per
        candidate with time step ``dt`` and ball-joint ``damping``.  Returns ``rpy`` (S, 3), ``base_position`` (S, 3), ``base_vel`` (S, 6),
        ``base_acc`` (S, 6) -- the base state arrays of the other candidate calls -- and with ``with_info`` ``att_state`` (S, 6): the
        attachment's rpy and angular velocity at each step, ``info`` (C, 2) int64: equilibrium iterations, clamp events.  Torch tensors when
        the states are on the device, NumPy arrays otherwise (``device_out`` overrides)."""
        s, keep, S, mem = self._joint_states(st)
        x = np.ascontiguousarray(x_std, dtype=np.float64)
        C = int(ncand)
        out_mem = mem if device_out is None else (FBR_DEVICE if device_out else FBR_HOST)
        shapes = {"rpy": (S, 3), "base_position": (S, 3), "base_vel": (S, 6), "base_acc": (S, 6)}
        if with_info:
            shapes["att_state"] = (S, 6)
        out = {k: self._out(None, shp, out_mem) for k, shp in shapes.items()}
        pinfo, info = None, None
        if with_info:
            if out_mem == FBR_DEVICE:
                import torch

                info = torch.empty((max(C, 1), 2), dtype=torch.int64, device=f"cuda:{self.device}")
                pinfo = info.data_ptr()
            else:
                info = np.empty((max(C, 1), 2), dtype=np.int64)
                pinfo = info.ctypes.data
        _check(self._lib.fbr_suspended_base_motion(self._h, ctypes.byref(s), C, x.ctypes.data_as(_dp), int(x.size), self._link_index(att_link),
                                                   float(dt), float(damping), out["rpy"][0].ptr, out["base_position"][0].ptr, out["base_vel"][0].ptr,
                                                   out["base_acc"][0].ptr, out["att_state"][0].ptr if with_info else None, pinfo, out_mem),
               "fbr_suspended_base_motion")
        res = {k: v[1] for k, v in out.items()}
        if with_info:
            res["info"] = info
        return res

    def suspended_records(self, st: dict, x_std, att_link, device_out: bool | None = None):
        """The (S, 39) per-sample records ``suspended_base_motion`` steps through (``fbr_suspended_records``; tests, tooling): composite
        inertia about the attachment origin (xx xy xz yy yz zz) | Coriolis coupling (3 x 3) | joint-motion moment | first mass moment | pose
        R (3 x 3), p and twist of the base link relative to the attachment frame, in the attachment link's axes."""
        s, keep, S, mem = self._joint_states(st)
        x = np.ascontiguousarray(x_std, dtype=np.float64)
        out_mem = mem if device_out is None else (FBR_DEVICE if device_out else FBR_HOST)
        r, ret = self._out(None, (S, 39), out_mem)
        _check(self._lib.fbr_suspended_records(self._h, ctypes.byref(s), x.ctypes.data_as(_dp), int(x.size), self._link_index(att_link), r.ptr, out_mem),
               "fbr_suspended_records")
        return ret

    def set_capsules(self, capsules, pairs) -> None:
        """Capsule collision set of the handle (``fbr_model_set_capsules``).  ``capsules``: a sequence of ``(link, p0, p1, radius)`` -- link
        an index into the topology's links or a link name, p0 / p1 in that link's frame -- or of objects with ``link`` / ``link_name``,
        ``p0_local``, ``p1_local``, ``radius`` (``flobaroid_amd.collision.Capsule``); ``pairs``: (P, 2) indices into that sequence.  Replaces
        the set in place; an empty ``capsules`` clears it."""
        names = list(self.topo.link_names)
        link, seg, rad = [], [], []
        for c in capsules:
            if hasattr(c, "radius"):
                l, p0, p1, r = (c.link if getattr(c, "link", None) is not None else c.link_name), c.p0_local, c.p1_local, c.radius
            else:
                l, p0, p1, r = c
            link.append(names.index(l) if isinstance(l, str) else int(l))
            seg.append(np.concatenate([np.asarray(p0, dtype=np.float64).reshape(3), np.asarray(p1, dtype=np.float64).reshape(3)]))
            rad.append(float(r))
        link = np.ascontiguousarray(link, dtype=np.int32)
        seg = np.ascontiguousarray(np.array(seg, dtype=np.float64).reshape(-1, 6))
        rad = np.ascontiguousarray(rad, dtype=np.float64)
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        _check(self._lib.fbr_model_set_capsules(self._h, int(link.size), link.ctypes.data_as(_ip), seg.ctypes.data_as(_dp), rad.ctypes.data_as(_dp),
                                                int(pr.shape[0]), pr.ctypes.data_as(_ip)), "fbr_model_set_capsules")
        self.num_capsules, self.num_capsule_pairs = int(link.size), int(pr.shape[0])

    def set_boxes(self, boxes, pairs, center_in_link_axes: bool = False) -> None:
        """Box collision set of the handle (``fbr_model_set_boxes``), independent of the capsule set.  ``boxes``: a sequence of
        ``(link, half, center, rot)`` -- link an index into the topology's links, a link name, or None / -1 for a world box; half extents;
        centre (robot box: offset from the link origin; world box: in the world); rot (3, 3) with the box axes as columns (world boxes; None
        otherwise) -- or of objects with ``link`` / ``link_name``, ``half``, ``center``, ``rot`` (``flobaroid_amd.collision.Box``);
        ``pairs``: (P, 2) indices into that sequence.  ``center_in_link_axes``: False places a robot box at ``p_link + center`` (the
        reference's sum in world axes), True at ``p_link + R_link center``.  Replaces the set in place; an empty ``boxes`` clears it."""
        names = list(self.topo.link_names)
        link, half, cen, rot, any_world = [], [], [], [], False
        for b in boxes:
            if hasattr(b, "half"):
                l, h, c, r = (b.link if getattr(b, "link", None) is not None else getattr(b, "link_name", None)), b.half, b.center, b.rot
            else:
                l, h, c, r = b
            l = -1 if l is None else (names.index(l) if isinstance(l, str) else int(l))
            link.append(l)
            half.append(np.asarray(h, dtype=np.float64).reshape(3))
            cen.append(np.asarray(c, dtype=np.float64).reshape(3))
            if l < 0 and r is None:
                raise ValueError("a world box needs its rotation")
            any_world |= l < 0
            rot.append(np.eye(3).reshape(9) if r is None else np.asarray(r, dtype=np.float64).reshape(9))
        link = np.ascontiguousarray(link, dtype=np.int32)
        half = np.ascontiguousarray(np.array(half, dtype=np.float64).reshape(-1, 3))
        cen = np.ascontiguousarray(np.array(cen, dtype=np.float64).reshape(-1, 3))
        rot = np.ascontiguousarray(np.array(rot, dtype=np.float64).reshape(-1, 9))
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        _check(self._lib.fbr_model_set_boxes(self._h, int(link.size), link.ctypes.data_as(_ip), half.ctypes.data_as(_dp), cen.ctypes.data_as(_dp),
                                             rot.ctypes.data_as(_dp) if any_world else None, int(bool(center_in_link_axes)), int(pr.shape[0]),
                                             pr.ctypes.data_as(_ip)), "fbr_model_set_boxes")
        self.num_boxes, self.num_box_pairs = int(link.size), int(pr.shape[0])

    def candidate_box_distances(self, st: dict, ncand: int, step: int = 3, base_pos=None, device_out: bool | None = None) -> dict:
        """Per candidate and box pair, the smallest signed box distance over every ``step``-th sample of the candidate and the sample index
        where it is reached (``fbr_candidate_box_distances``): ``{"dist": (C, P), "idx": (C, P) int64}``, arguments and rules as for
        ``candidate_capsule_distances``.  Separated boxes: the exact Euclidean distance; overlapping: minus the minimum translation."""
        return self._candidate_distances("fbr_candidate_box_distances", int(getattr(self, "num_box_pairs", 0)), st, ncand, step, base_pos, device_out)

    def set_hulls(self, hulls, pairs, offset_in_link_axes: bool = False, meshes=None, large: bool = False, large_meshes: bool = False) -> None:
        """Convex-hull collision set of the handle (``fbr_model_set_hulls``), independent of the capsule and the box set.  ``hulls``: a
        sequence of ``flobaroid_amd.collision.Hull`` (``link_name`` None: a world hull with ``rot``), or of tuples ``(link, offset, rot,
        vertices, planes, edges)`` -- link an index, a name, or None / -1; the tables as ``Hull`` derives them.  ``pairs``: (P, 2) indices
        into that sequence.  ``offset_in_link_axes``: False places a robot hull at ``p_link + offset`` (the reference's sum in world
        axes), True at ``p_link + R_link offset``.  Replaces the set in place; an empty ``hulls`` clears it.  ``meshes``: what
        ``set_hull_meshes`` takes, attached to the new set (None: the new set has no meshes, whatever the one before had).  ``large``: False
        is ``fbr_model_set_hulls``, at most ``FBR_MAX_HULL_VERTICES`` (128) vertices a hull; True is ``fbr_model_set_large_hulls``, up to
        ``FBR_MAX_LARGE_HULL_VERTICES`` (1024): distances only -- no ``meshes`` (ValueError) unless ``large_meshes``, and the gradient
        calls refuse the set while one of its hulls has more than 128 vertices.  ``large_meshes``: attach ``meshes`` through
        ``set_large_hull_meshes`` (up to ``FBR_MAX_LARGE_MESH_TRIANGLES`` triangles a mesh, on small or large hulls; the gradients of such a
        set come from ``large_mesh_distance_gradients``)."""
        if large and meshes and not large_meshes:
            raise ValueError("set_hulls(large=True): triangle meshes on a set of large hulls are not built (meshes= needs large=False)")
        names = list(self.topo.link_names)
        link, off, rot, V, F, E, any_world = [], [], [], [], [], [], False
        for h in hulls:
            if hasattr(h, "vertices"):
                l, o, r, v, f, e = h.link_name, h.offset, h.rot, h.vertices, h.planes, h.edges
            else:
                l, o, r, v, f, e = h
            l = -1 if l is None else (names.index(l) if isinstance(l, str) else int(l))
            if l < 0 and r is None:
                raise ValueError("a world hull needs its rotation")
            any_world |= l < 0
            link.append(l)
            off.append(np.asarray(o, dtype=np.float64).reshape(3))
            rot.append(np.eye(3).reshape(9) if r is None else np.asarray(r, dtype=np.float64).reshape(9))
            V.append(np.asarray(v, dtype=np.float64).reshape(-1, 3))
            F.append(np.asarray(f, dtype=np.float64).reshape(-1, 4))
            E.append(np.asarray(e, dtype=np.int32).reshape(-1, 4))
        cat = lambda parts, w, t: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, w)), dtype=t)  # noqa: E731
        beg = lambda parts: np.ascontiguousarray(np.cumsum([0] + [len(x) for x in parts]), dtype=np.int32)  # noqa: E731
        link = np.ascontiguousarray(link, dtype=np.int32)
        off, rot = cat([o[None] for o in off], 3, np.float64), cat([r[None] for r in rot], 9, np.float64)
        verts, planes, edges = cat(V, 3, np.float64), cat(F, 4, np.float64), cat(E, 4, np.int32)
        vbeg, fbeg, ebeg = beg(V), beg(F), beg(E)
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        entry = "fbr_model_set_large_hulls" if large else "fbr_model_set_hulls"
        _check(getattr(self._lib, entry)(self._h, int(link.size), link.ctypes.data_as(_ip), off.ctypes.data_as(_dp),
                                         rot.ctypes.data_as(_dp) if any_world else None, int(bool(offset_in_link_axes)), vbeg.ctypes.data_as(_ip),
                                         verts.ctypes.data_as(_dp), fbeg.ctypes.data_as(_ip), planes.ctypes.data_as(_dp), ebeg.ctypes.data_as(_ip),
                                         edges.ctypes.data_as(_ip), int(pr.shape[0]), pr.ctypes.data_as(_ip)), entry)
        self.num_hulls, self.num_hull_pairs, self.num_hull_meshes = int(link.size), int(pr.shape[0]), 0
        if meshes:
            (self.set_large_hull_meshes if large_meshes else self.set_hull_meshes)(meshes)

    def set_large_hull_meshes(self, meshes) -> None:
        """``set_hull_meshes`` for meshes of up to ``FBR_MAX_LARGE_MESH_TRIANGLES`` (8192) triangles, on a set of ``set_hulls`` with or
        without ``large=True`` (``fbr_model_set_large_hull_meshes``): KUKA LWR4's visual meshes, ``collisionMode: "full"`` on a robot
        without collision meshes.  The library builds a bounding-sphere tree per mesh and ``candidate_hull_distances`` walks the two
        trees of a pair for the 64 samples of a wave together; the values have the bits of the brute force over all triangle pairs.  No
        cap on the triangle pairs of a pair.  ``large_mesh_distance_gradients`` serves the gradients of such a set; the three other hull
        gradient calls refuse it while such meshes are attached."""
        self._set_meshes("fbr_model_set_large_hull_meshes", meshes)

    def set_hull_meshes(self, meshes) -> None:
        """Triangle meshes on hulls of the set ``set_hulls`` put in place (``fbr_model_set_hull_meshes``; the reference's ``fullMeshLinks``
        and ``collisionMode: "full"``).  ``meshes``: ``{hull index: triangles (T, 3, 3)}`` in the hull's axes (``collision_set(...,
        meshes=)["meshes"]``), or a sequence of such pairs.  ``candidate_hull_distances`` then serves every pair with a meshed hull by the
        mesh routine: the minimum over the triangles, exactly 0.0 where they touch or intersect, never negative.  An empty ``meshes``
        clears the attachments, and so does every later ``set_hulls``; ``hull_distance_gradients`` refuses a set with meshes,
        ``mesh_distance_gradients`` serves it."""
        self._set_meshes("fbr_model_set_hull_meshes", meshes)

    def _set_meshes(self, entry: str, meshes) -> None:
        items = list(meshes.items()) if hasattr(meshes, "items") else list(meshes or [])
        tri = [np.asarray(t, dtype=np.float64).reshape(-1, 9) for _, t in items]
        hull = np.ascontiguousarray([int(h) for h, _ in items], dtype=np.int32)
        tbeg = np.ascontiguousarray(np.cumsum([0] + [len(t) for t in tri]), dtype=np.int32)
        tris = np.ascontiguousarray(np.concatenate(tri) if tri else np.zeros((0, 9)))
        _check(getattr(self._lib, entry)(self._h, len(items), hull.ctypes.data_as(_ip), tbeg.ctypes.data_as(_ip), tris.ctypes.data_as(_dp)), entry)
        self.num_hull_meshes = len(items)

    def candidate_hull_distances(self, st: dict, ncand: int, step: int = 3, base_pos=None, device_out: bool | None = None) -> dict:
        """Per candidate and hull pair, the smallest signed hull distance over every ``step``-th sample of the candidate and the sample
        index where it is reached (``fbr_candidate_hull_distances``): ``{"dist": (C, P), "idx": (C, P) int64}``, arguments and rules as
        for ``candidate_box_distances``.  Separated hulls: the Euclidean distance; touching or overlapping: minus the minimum translation.
        Pairs with a meshed hull (``set_hull_meshes``): the mesh distance, 0.0 where they touch or intersect."""
        return self._candidate_distances("fbr_candidate_hull_distances", int(getattr(self, "num_hull_pairs", 0)), st, ncand, step, base_pos, device_out)

    def candidate_capsule_distances(self, st: dict, ncand: int, step: int = 3, base_pos=None, device_out: bool | None = None) -> dict:
        """Per candidate and capsule pair, the smallest capsule distance over every ``step``-th sample of the candidate and the sample index
        (inside the candidate) where it is reached (``fbr_candidate_capsule_distances``): ``{"dist": (C, P), "idx": (C, P) int64}``; 1e10 / -1
        for a pair no sample won (NaN poses).  ``st`` needs ``q`` and, with a floating base, ``rpy`` only; ``base_pos`` (S, 3) places the
        base (None: the origin).  Torch tensors when the states are on the device, NumPy arrays otherwise (``device_out`` overrides)."""
        return self._candidate_distances("fbr_candidate_capsule_distances", int(getattr(self, "num_capsule_pairs", 0)), st, ncand, step, base_pos,
                                         device_out)

    def _candidate_distances(self, entry: str, P: int, st: dict, ncand: int, step: int, base_pos, device_out) -> dict:
        """the capsule and the box call share their arguments: ``entry`` names the library's function, ``P`` the pairs of its set"""
        q = _Ref(st["q"], None, "q")
        if len(q.obj.shape) != 2 or q.obj.shape[1] != self.n:
            raise ValueError(f"q: expected (S, {self.n}), got {tuple(q.obj.shape)}")
        S = int(q.obj.shape[0])
        rpy = _Ref(st.get("rpy", st.get("base_rpy")), (S, 3), "base_rpy") if self.floating else _Ref(None)
        bp = _Ref(base_pos, (S, 3), "base_pos") if self.floating else _Ref(None)
        mem = _same_space([q, rpy, bp])
        if mem == FBR_DEVICE:
            self._sync_torch()
        s = fbr_states()
        s.num_samples, s.mem, s.q, s.base_rpy = S, mem, q.ptr, rpy.ptr
        C = int(ncand)
        shape = (max(C, 1), P)
        out_mem = mem if device_out is None else (FBR_DEVICE if device_out else FBR_HOST)
        if out_mem == FBR_DEVICE:
            import torch

            val = torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.device}")
            idx = torch.empty(shape, dtype=torch.int64, device=f"cuda:{self.device}")
            pv, pi = val.data_ptr(), idx.data_ptr()
        else:
            val, idx = np.empty(shape), np.empty(shape, dtype=np.int64)
            pv, pi = val.ctypes.data, idx.ctypes.data
        _check(getattr(self._lib, entry)(self._h, ctypes.byref(s), bp.ptr, C, int(step), pv, pi, out_mem), entry)
        return {"dist": val, "idx": idx}

    def _index_array(self, x, shape, mem, name, dtype=np.int64):
        """an int64 (or ``dtype`` int32) index array in the memory space ``mem``: (keep-alive object, pointer)"""
        if mem == FBR_DEVICE:
            import torch

            t = torch.as_tensor(x, device=f"cuda:{self.device}").to(torch.int64 if dtype == np.int64 else torch.int32).contiguous()
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
            return t, t.data_ptr()
        a = np.ascontiguousarray(x.cpu().numpy() if _is_torch(x) else x, dtype=dtype)
        if a.shape != tuple(shape):
            raise ValueError(f"{name}: expected shape {shape}, got {a.shape}")
        return a, a.ctypes.data

    def _to_space(self, x, mem):
        """a float64 array brought to the memory space ``mem`` (None stays None)"""
        if x is None:
            return None
        if mem == FBR_DEVICE:
            import torch

            return torch.as_tensor(x, dtype=torch.float64, device=f"cuda:{self.device}")
        return x.cpu().numpy() if _is_torch(x) else np.asarray(x, dtype=np.float64)

    def capsule_distance_gradients(self, st: dict, ncand: int, sample, scale=None, pose_sample=None, base_pos=None,
                                   device_out: bool | None = None) -> dict:
        """Capsule distance and its derivative with respect to the joint positions at one chosen configuration per candidate and pair
        (``fbr_capsule_distance_gradients``): ``{"dist": (C, P), "grad_q": (C, P, n)}``.  ``sample`` (C, P) int: the sample inside the
        candidate whose row of ``q`` is evaluated (-1: none -- 1e10 and a zero row); ``scale`` (C, P) or None: the configuration is
        ``scale * q[sample]``; ``pose_sample`` (C, P) or None: the sample whose base pose is used (floating base).  ``grad_q`` is the
        derivative with respect to the EVALUATED configuration; joints off the tree path between a pair's links are exact zeros.  ``st``,
        ``base_pos`` and the result's memory space as for ``candidate_capsule_distances``; the index and scale arrays are brought to the
        memory space of the states."""
        return self._distance_gradients("fbr_capsule_distance_gradients", int(getattr(self, "num_capsule_pairs", 0)), (), st, ncand, sample, scale,
                                        pose_sample, base_pos, device_out)

    def box_distance_gradients(self, st: dict, ncand: int, sample, scale=None, pose_sample=None, base_pos=None, epsilon: float = 1e-7,
                               device_out: bool | None = None) -> dict:
        """Signed box distance and its central-difference derivative with respect to the joint positions at one chosen configuration per
        candidate and box pair (``fbr_box_distance_gradients``): ``{"dist": (C, P_box), "grad_q": (C, P_box, n)}``, arguments and rules as
        for ``capsule_distance_gradients``.  ``epsilon``: the step of the difference (the reference's ``analyticalGradientEpsilon``).  Joints
        off the tree path between a pair's links, joints above both links and fixed joints are exact zeros.  A pair of two robot boxes
        with ``center_in_link_axes`` does not depend on the base pose and returns the bits of a stationary base (so do the hull and mesh
        calls below with ``offset_in_link_axes``)."""
        return self._distance_gradients("fbr_box_distance_gradients", int(getattr(self, "num_box_pairs", 0)), (float(epsilon),), st, ncand, sample,
                                        scale, pose_sample, base_pos, device_out)

    def hull_distance_gradients(self, st: dict, ncand: int, sample, scale=None, pose_sample=None, base_pos=None, epsilon: float = 1e-7,
                                device_out: bool | None = None) -> dict:
        """Signed hull distance and its central-difference derivative with respect to the joint positions at one chosen configuration per
        candidate and hull pair (``fbr_hull_distance_gradients``): ``{"dist": (C, P_hull), "grad_q": (C, P_hull, n)}``, arguments and rules
        as for ``box_distance_gradients``; a hull's offset follows ``offset_in_link_axes`` of ``set_hulls`` as a box centre follows
        ``center_in_link_axes``."""
        return self._distance_gradients("fbr_hull_distance_gradients", int(getattr(self, "num_hull_pairs", 0)), (float(epsilon),), st, ncand, sample,
                                        scale, pose_sample, base_pos, device_out)

    def mesh_distance_gradients(self, st: dict, ncand: int, sample, scale=None, pose_sample=None, base_pos=None, epsilon: float = 1e-7,
                                device_out: bool | None = None) -> dict:
        """``hull_distance_gradients`` for a hull set with triangle meshes attached (``set_hull_meshes``; ``fbr_mesh_distance_gradients``):
        ``{"dist": (C, P_hull), "grad_q": (C, P_hull, n)}`` over ALL pairs of the set, arguments and rules as there.  A pair without a mesh
        returns the bytes ``hull_distance_gradients`` gives it from the same set without meshes; a pair with one the mesh distance and its
        central differences over ``epsilon``.  A mesh distance is exactly 0.0 on contact and never negative, so a pair in intersection has
        an exactly zero row: a mesh carries no penetration depth.  A set without meshes is refused (``hull_distance_gradients`` serves it)."""
        return self._distance_gradients("fbr_mesh_distance_gradients", int(getattr(self, "num_hull_pairs", 0)), (float(epsilon),), st, ncand, sample,
                                        scale, pose_sample, base_pos, device_out)

    def large_hull_distance_gradients(self, st: dict, ncand: int, sample, scale=None, pose_sample=None, base_pos=None, epsilon: float = 1e-7,
                                      device_out: bool | None = None) -> dict:
        """``hull_distance_gradients`` for a hull set installed with ``set_hulls(..., large=True)`` (``fbr_large_hull_distance_gradients``):
        ``{"dist": (C, P_hull), "grad_q": (C, P_hull, n)}`` over ALL pairs of the set, arguments and rules as there.  A pair of two hulls
        of at most ``FBR_MAX_HULL_VERTICES`` vertices returns the bytes ``hull_distance_gradients`` gives it from a set without large
        hulls; every other pair (every pair with option ``hull_large_all`` = 1) the same central differences with the facet pass of a
        touching stencil point shared by a wave.  A set installed without ``large=True`` is refused."""
        return self._distance_gradients("fbr_large_hull_distance_gradients", int(getattr(self, "num_hull_pairs", 0)), (float(epsilon),), st, ncand,
                                        sample, scale, pose_sample, base_pos, device_out)

    def large_mesh_distance_gradients(self, st: dict, ncand: int, sample, scale=None, pose_sample=None, base_pos=None, epsilon: float = 1e-7,
                                      device_out: bool | None = None) -> dict:
        """``mesh_distance_gradients`` for a hull set -- of ``set_hulls`` with or without ``large=True`` -- with meshes attached through
        ``set_large_hull_meshes`` (``fbr_large_mesh_distance_gradients``): ``{"dist": (C, P_hull), "grad_q": (C, P_hull, n)}`` over ALL pairs of
        the set, arguments and rules as there.  A pair of two small hulls without a mesh returns the bytes of ``hull_distance_gradients``,
        a pair with a hull above ``FBR_MAX_HULL_VERTICES`` vertices and no mesh those of ``large_hull_distance_gradients``, each from the set
        without meshes; a pair with a mesh the mesh distance through the trees and its central differences over ``epsilon``, with the
        bytes ``mesh_distance_gradients`` gives where the meshes fit both attachments.  Option ``mesh_grad_order`` (1: candidate-major, 2:
        slot-major, 0: the default) orders the entries of a wave of the tree stage and never changes a value; option ``hull_large_all`` has
        no effect.  A set without such an attachment is refused by the name of the call that serves it."""
        return self._distance_gradients("fbr_large_mesh_distance_gradients", int(getattr(self, "num_hull_pairs", 0)), (float(epsilon),), st, ncand,
                                        sample, scale, pose_sample, base_pos, device_out)

    def _distance_gradients(self, entry: str, P: int, extra: tuple, st: dict, ncand: int, sample, scale, pose_sample, base_pos, device_out) -> dict:
        """the capsule, the box, the hull and the mesh call share their arguments: ``entry`` names the library's function, ``P`` the pairs of its set, ``extra``
        what the function takes between ``pose_sample`` and the outputs"""
        q = _Ref(st["q"], None, "q")
        if len(q.obj.shape) != 2 or q.obj.shape[1] != self.n:
            raise ValueError(f"q: expected (S, {self.n}), got {tuple(q.obj.shape)}")
        S = int(q.obj.shape[0])
        rpy = _Ref(st.get("rpy", st.get("base_rpy")), (S, 3), "base_rpy") if self.floating else _Ref(None)
        bp = _Ref(base_pos, (S, 3), "base_pos") if self.floating else _Ref(None)
        mem = _same_space([q, rpy, bp])
        if mem == FBR_DEVICE:
            self._sync_torch()
        s = fbr_states()
        s.num_samples, s.mem, s.q, s.base_rpy = S, mem, q.ptr, rpy.ptr
        C = int(ncand)
        shape = (max(C, 1), P)
        smp, psmp = self._index_array(sample, shape, mem, "sample")
        pose, ppose = (None, None) if pose_sample is None else self._index_array(pose_sample, shape, mem, "pose_sample")
        sc = _Ref(self._to_space(scale, mem), shape, "scale")
        out_mem = mem if device_out is None else (FBR_DEVICE if device_out else FBR_HOST)
        rd, dist = self._out(None, shape, out_mem)
        rg, grad = self._out(None, shape + (self.n,), out_mem)
        _check(getattr(self._lib, entry)(self._h, ctypes.byref(s), bp.ptr, C, psmp, sc.ptr, ppose, *extra, rd.ptr, rg.ptr, out_mem), entry)
        return {"dist": dist, "grad_q": grad}

    def fourier_position_chain(self, wf, a, b, sample, grad_q, freq: float, scale=None, q_range=None, device_out: bool | None = None):
        """Rows of position sensitivities ``grad_q`` (C, R, n), row r of candidate c taken at time ``sample[c, r] / freq``, chained with the
        position Jacobian of the series of ``fourier_states`` (``fbr_fourier_position_chain``): a (C, R, 1 + 2 n + 2 n nharm) array in the
        column layout of ``fourier_gradient``, entry = ``scale[c, r] * sum_d grad_q[c, r, d] * dq_d/dp``; rows with ``sample`` < 0 are
        zero.  A CUDA tensor when ``grad_q`` is (``device_out`` overrides), else NumPy; ``sample`` and ``scale`` are brought to its space."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        C, n, nh = a.shape
        if n != self.n or b.shape != a.shape:
            raise ValueError(f"a / b: expected (C, {self.n}, nharm)")
        wf = np.ascontiguousarray(np.broadcast_to(np.asarray(wf, dtype=np.float64), (C,)))
        qr = None if q_range is None else np.ascontiguousarray(q_range, dtype=np.float64).reshape(C, n)
        g = _Ref(grad_q, None, "grad_q")
        if len(g.obj.shape) != 3 or g.obj.shape[0] != C or g.obj.shape[2] != n:
            raise ValueError(f"grad_q: expected ({C}, R, {n}), got {tuple(g.obj.shape)}")
        R = int(g.obj.shape[1])
        mem = g.mem
        if mem == FBR_DEVICE:
            self._sync_torch()
        smp, psmp = self._index_array(sample, (C, R), mem, "sample")
        sc = _Ref(self._to_space(scale, mem), (C, R), "scale")
        out_mem = mem if device_out is None else (FBR_DEVICE if device_out else FBR_HOST)
        r, ret = self._out(None, (C, R, 1 + 2 * n + 2 * n * nh), out_mem)
        _check(self._lib.fbr_fourier_position_chain(self._h, C, R, nh, float(freq), wf.ctypes.data_as(_dp), a.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                                    None if qr is None else qr.ctypes.data_as(_dp), psmp, sc.ptr, g.ptr, mem, r.ptr, r.mem),
               "fbr_fourier_position_chain")
        return ret

    def fourier_state_chain(self, wf, a, b, sample, freq: float, grad_q=None, grad_dq=None, grad_ddq=None, scale=None, q_range=None,
                            device_out: bool | None = None):
        """``fourier_position_chain`` for rows with sensitivities to the joint velocities and accelerations as well
        (``fbr_fourier_state_chain``): entry = ``scale[c, r] * sum_d (grad_q[c, r, d] * dq_d/dp + grad_dq[c, r, d] * d(dq_d)/dp +
        grad_ddq[c, r, d] * d(ddq_d)/dp)`` at time ``sample[c, r] / freq``, every derivative analytic; each of ``grad_q`` / ``grad_dq`` /
        ``grad_ddq`` (C, R, n) may be None (zero), at least one is given and all live in one memory space.  Equal to
        ``fourier_position_chain`` entry for entry when only ``grad_q`` is given."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        C, n, nh = a.shape
        if n != self.n or b.shape != a.shape:
            raise ValueError(f"a / b: expected (C, {self.n}, nharm)")
        wf = np.ascontiguousarray(np.broadcast_to(np.asarray(wf, dtype=np.float64), (C,)))
        qr = None if q_range is None else np.ascontiguousarray(q_range, dtype=np.float64).reshape(C, n)
        given = [x for x in (grad_q, grad_dq, grad_ddq) if x is not None]
        if not given or len(given[0].shape) != 3 or given[0].shape[0] != C or given[0].shape[2] != n:
            raise ValueError(f"grad_q / grad_dq / grad_ddq: at least one array ({C}, R, {n})")
        R = int(given[0].shape[1])
        g = [_Ref(x, (C, R, n), name) if x is not None else _Ref(None) for x, name in ((grad_q, "grad_q"), (grad_dq, "grad_dq"), (grad_ddq, "grad_ddq"))]
        mem = _same_space(g)
        if mem == FBR_DEVICE:
            self._sync_torch()
        smp, psmp = self._index_array(sample, (C, R), mem, "sample")
        sc = _Ref(self._to_space(scale, mem), (C, R), "scale")
        out_mem = mem if device_out is None else (FBR_DEVICE if device_out else FBR_HOST)
        r, ret = self._out(None, (C, R, 1 + 2 * n + 2 * n * nh), out_mem)
        _check(self._lib.fbr_fourier_state_chain(self._h, C, R, nh, float(freq), wf.ctypes.data_as(_dp), a.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                                 None if qr is None else qr.ctypes.data_as(_dp), psmp, sc.ptr, g[0].ptr, g[1].ptr, g[2].ptr, mem, r.ptr,
                                                 r.mem), "fbr_fourier_state_chain")
        return ret

    def predict(self, st: dict, x, out=None):
        s, keep, S, mem = self._states(st)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.size != self.cols:
            raise ValueError(f"x must have {self.cols} entries")
        r, ret = self._out(out, (S, self.rows), mem)
        _check(self._lib.fbr_predict(self._h, ctypes.byref(s), x.ctypes.data_as(_dp), r.ptr, r.mem), "fbr_predict")
        return ret

    def contact_torques(self, st: dict, frame: str, wrench, out=None):
        t = self.topo
        if frame in t.frames:
            link, fR, fp = t.frames[frame]["link"], t.frames[frame]["R"], t.frames[frame]["p"]
        elif frame in t.link_names:
            link, fR, fp = t.link_names.index(frame), np.eye(3), np.zeros(3)
        else:
            raise KeyError(f"unknown frame '{frame}'")
        s, keep, S, mem = self._states(st, need_vel=False)
        w = _Ref(wrench, (S, 6), "wrench")
        if w.mem != mem:
            raise ValueError("wrench must live in the same memory space as the states")
        fR = np.ascontiguousarray(fR, dtype=np.float64).reshape(-1)
        fp = np.ascontiguousarray(fp, dtype=np.float64).reshape(-1)
        r, ret = self._out(out, (S, self.rows), mem)
        _check(
            self._lib.fbr_contact_torques(self._h, ctypes.byref(s), int(link), fR.ctypes.data_as(_dp),
                                          fp.ctypes.data_as(_dp), w.ptr, r.ptr, r.mem),
            "fbr_contact_torques",
        )
        return ret

    def _rhs(self, rhs, w, S, mem):
        k = 0
        rr = _Ref(None)
        if rhs is not None:
            if not _is_torch(rhs):
                rhs = np.asarray(rhs, dtype=np.float64)
            ncol = int(rhs.shape[-1]) if rhs.ndim >= 2 else 1  # (an empty batch cannot infer the column count by reshape)
            rhs2 = rhs.reshape(S * self.rows, ncol)
            k = int(rhs2.shape[1])
            rr = _Ref(rhs2, (S * self.rows, k), "rhs")
            if rr.mem != mem:
                raise ValueError("rhs must live in the same memory space as the states")
        wr = _Ref(None)
        if w is not None:
            w2 = w.reshape(S * self.rows) if _is_torch(w) else np.asarray(w, dtype=np.float64).reshape(S * self.rows)
            wr = _Ref(w2, (S * self.rows,), "w")
            if wr.mem != mem:
                raise ValueError("w must live in the same memory space as the states")
        return rr, wr, k

    def gram(self, st: dict, rhs=None, w=None, out=None, accumulate: bool = False):
        """Raw Gram [Y|rhs]^T diag(w)^2 [Y|rhs], shape (cols+k, cols+k)."""
        s, keep, S, mem = self._states(st)
        rr, wr, k = self._rhs(rhs, w, S, mem)
        Pa = self.cols + k
        r, ret = self._out(out, (Pa, Pa), mem)
        _check(
            self._lib.fbr_gram_accumulate(self._h, ctypes.byref(s), rr.ptr, k, wr.ptr, r.ptr, r.mem, int(bool(accumulate))),
            "fbr_gram_accumulate",
        )
        return ret

    def gram_submit(self, st: dict, out, rhs=None, w=None, accumulate: bool = False) -> int:
        """``gram`` without waiting (``fbr_gram_submit``): ``out`` is a CUDA tensor, the inputs CUDA tensors or PINNED host tensors
        (staged chunk by chunk on a copy stream); result in ``out`` after ``wait(ticket)``.  The caller keeps ``st`` / ``rhs`` / ``w`` /
        ``out`` alive and untouched until then; at most two submissions are in flight."""
        s, keep, S, mem = self._states(st)
        rr, wr, k = self._rhs(rhs, w, S, mem)
        Pa = self.cols + k
        r, _ = self._out(out, (Pa, Pa), mem)
        if r.mem != FBR_DEVICE:
            raise ValueError("gram_submit needs a CUDA tensor for the output")
        t = ctypes.c_int64(-1)
        _check(self._lib.fbr_gram_submit(self._h, ctypes.byref(s), rr.ptr, k, wr.ptr, r.ptr, int(bool(accumulate)), ctypes.byref(t)),
               "fbr_gram_submit")
        # the GPU reads the arrays handed to the library until wait(): contiguous copies / reshapes made on the way (``_Ref``, ``_rhs``)
        # would otherwise go back to torch's allocator on return and could be reused while still being read
        self._keep_inflight(int(t.value), (keep, rr, wr, r))
        return int(t.value)

    def _keep_inflight(self, ticket: int, refs) -> None:
        infl = self.__dict__.setdefault("_inflight", {})
        infl[ticket] = refs
        for old in [k_ for k_ in infl if k_ < ticket - 1]:  # (a third submission has waited for the oldest inside the library)
            del infl[old]

    def wait(self, ticket: int = -1) -> None:
        """Block until the submission ``ticket`` (default: everything submitted) is complete."""
        try:
            _check(self._lib.fbr_wait(self._h, int(ticket)), "fbr_wait")
        finally:
            infl = self.__dict__.get("_inflight", {})
            for k_ in [k_ for k_ in infl if ticket < 0 or k_ <= ticket]:
                del infl[k_]

    def tsqr_submit(self, st: dict, out, rhs=None, w=None, R_in=None, cols=None) -> int:
        """``tsqr`` without waiting (``fbr_tsqr_submit``): CUDA tensors only; result in ``out`` after ``wait(ticket)``.  At most two
        submissions (of either kind) are in flight; consecutive TSQR submissions overlap the next one's kinematics / first regressor
        chunk with the merge trees of the one before."""
        s, keep, S, mem = self._states(st)
        rr, wr, k = self._rhs(rhs, w, S, mem)
        ca = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
        Pa = (self.cols if ca is None else int(ca.size)) + k
        r, _ = self._out(out, (Pa, Pa), mem)
        rin = _Ref(R_in, (Pa, Pa), "R_in") if R_in is not None else _Ref(None)
        if mem != FBR_DEVICE or r.mem != FBR_DEVICE or (rin.mem is not None and rin.mem != FBR_DEVICE):
            raise ValueError("tsqr_submit needs CUDA tensors for the states, rhs, weights, R_in and the output")
        t = ctypes.c_int64(-1)
        _check(self._lib.fbr_tsqr_submit(self._h, ctypes.byref(s), None if ca is None else ca.ctypes.data_as(_ip), 0 if ca is None else int(ca.size),
                                         rr.ptr, k, wr.ptr, rin.ptr, r.ptr, ctypes.byref(t)), "fbr_tsqr_submit")
        self._keep_inflight(int(t.value), (keep, rr, wr, rin, r, ca))
        return int(t.value)

    def gram_grouped(self, st: dict, ngroups: int, rhs=None, w=None, out=None):
        """One raw Gram per group of S / ngroups consecutive samples, shape (ngroups, cols+k, cols+k), in one pass."""
        s, keep, S, mem = self._states(st)
        if ngroups < 1 or S % ngroups:
            raise ValueError("the number of samples must be a multiple of ngroups")
        rr, wr, k = self._rhs(rhs, w, S, mem)
        Pa = self.cols + k
        r, ret = self._out(out, (int(ngroups), Pa, Pa), mem)
        _check(self._lib.fbr_gram_grouped(self._h, ctypes.byref(s), int(ngroups), rr.ptr, k, wr.ptr, r.ptr, r.mem), "fbr_gram_grouped")
        return ret

    def fd_scores(self, st: dict, W, eps: float, out=None):
        """Weighted regressor scores sum(W_s * Y) of every sample's baseline state and its 3n states perturbed by +eps
        in q_d, dq_d, ddq_d: shape (S, 1 + 3n) (analyticalGradient.py:92-185 without the per-sample Python loop)."""
        s, keep, S, mem = self._states(st)
        Wr = _Ref(W if _is_torch(W) else np.asarray(W, dtype=np.float64).reshape(S * self.rows, self.cols), (S * self.rows, self.cols), "W")
        if Wr.mem != mem:
            raise ValueError("W must live in the same memory space as the states")
        r, ret = self._out(out, (S, 1 + 3 * self.topo.num_dofs), mem)
        _check(self._lib.fbr_fd_scores(self._h, ctypes.byref(s), Wr.ptr, float(eps), r.ptr, r.mem), "fbr_fd_scores")
        return ret

    def fourier_states(self, wf, a, b, q_offset, T: int, freq: float, q_range=None, device: bool = True) -> dict:
        """q, dq, ddq of C candidate trajectories x T samples from their Fourier coefficients (``fbr_fourier_states``): ``wf`` (C,),
        ``a`` / ``b`` (C, n, nharm), ``q_offset`` (C, n), ``q_range`` (C, n) or None.  Returns {"q", "dq", "ddq"} of shape (C * T, n) --
        CUDA tensors (``device=True``: they stay in HBM for ``gram_grouped``) or NumPy arrays."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        C, n, nh = a.shape
        if n != self.n or b.shape != a.shape:
            raise ValueError(f"a / b: expected (C, {self.n}, nharm)")
        wf = np.ascontiguousarray(np.broadcast_to(np.asarray(wf, dtype=np.float64), (C,)))
        qo = np.ascontiguousarray(q_offset, dtype=np.float64).reshape(C, n)
        qr = None if q_range is None else np.ascontiguousarray(q_range, dtype=np.float64).reshape(C, n)
        outs, refs = [], []
        for _ in range(3):
            r, ret = self._out(None, (C * int(T), n), FBR_DEVICE if device else FBR_HOST)
            outs.append(ret)
            refs.append(r)
        _check(self._lib.fbr_fourier_states(self._h, C, int(T), nh, float(freq), wf.ctypes.data_as(_dp), a.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                            qo.ctypes.data_as(_dp), None if qr is None else qr.ctypes.data_as(_dp), refs[0].ptr, refs[1].ptr, refs[2].ptr,
                                            refs[0].mem), "fbr_fourier_states")
        return {"q": outs[0], "dq": outs[1], "ddq": outs[2]}

    def regressor_weights(self, st: dict, ngroups: int, C, cols=None, out=None):
        """Weight rows of the D-optimality gradient (``fbr_regressor_weights``): (S * rows, cols_of_the_model) with
        ``W[s][:, cols] = Y_s[:, cols] @ C[g]`` for the sample's group g (``ngroups`` equal groups of consecutive samples) and exact zeros in
        every other column -- the ``W`` that ``fd_scores`` takes.  ``C`` (ngroups, ncols, ncols), general; ``cols=None``: every column.
        ``C`` may be a NumPy array or a tensor: it is brought to the memory space of the states."""
        s, keep, S, mem = self._states(st)
        ca = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        nc = self.cols if ca is None else int(ca.size)
        G = int(ngroups)
        if _is_torch(C):
            C = C.reshape(max(G, 1), nc, nc)
            if mem == FBR_HOST:
                C = C.cpu()
            elif C.device.type != "cuda":
                C = C.to(f"cuda:{self.device}")
        else:
            C = np.ascontiguousarray(C, dtype=np.float64).reshape(max(G, 1), nc, nc)
            if mem == FBR_DEVICE:
                import torch

                C = torch.from_numpy(C).to(f"cuda:{self.device}")
        Cr = _Ref(C, (max(G, 1), nc, nc), "C")
        r, ret = self._out(out, (S * self.rows, self.cols), mem)
        _check(self._lib.fbr_regressor_weights(self._h, ctypes.byref(s), G, None if ca is None else ca.ctypes.data_as(_ip), nc, Cr.ptr, r.ptr, r.mem),
               "fbr_regressor_weights")
        return ret

    def dopt_terms(self, G, cols, reg: float = 1e-4, prior=None, scale=None, eigenvalues: bool = False, weights: bool = False,
                   device_out: bool | None = None) -> dict:
        """The D-optimality arithmetic of C candidates from their Grams ``G`` (C, Pa, Pa) (``gram_grouped``) on the device
        (``fbr_dopt_terms``): per candidate the eigenvalues of ``M = G[cols, cols] (+ prior)`` (lower triangle, as ``eigvalsh``) and
        ``neg_log_det``, ``lambda_max``, ``delta = reg * max(lambda_max, 1e-30)``, ``n_observable`` (int64), ``status`` (int32; bit 1: a
        non-finite entry, that candidate's numbers are NaN; bit 2: the factorisation met a pivot that is not positive).  ``eigenvalues``:
        also ``eig`` (C, ncols) ascending.  ``weights``: also ``Cmat`` (C, ncols, ncols) = -2 scale (M + delta I)^-1, exactly symmetric,
        what ``regressor_weights`` takes; a candidate with a non-zero status then raises ``np.linalg.LinAlgError``.  ``cols``: distinct,
        any order; ``prior`` (ncols, ncols) is brought to the memory space of ``G``; ``scale``: a number or one per candidate.
        The arrays are tensors when ``G`` is a CUDA tensor and NumPy arrays otherwise (``device_out`` overrides)."""
        import torch

        Gr = _Ref(G, name="G")
        if len(Gr.obj.shape) != 3 or Gr.obj.shape[1] != Gr.obj.shape[2]:
            raise ValueError(f"G: expected (C, Pa, Pa), got {tuple(Gr.obj.shape)}")
        C, Pa = int(Gr.obj.shape[0]), int(Gr.obj.shape[1])
        mem = Gr.mem
        if mem == FBR_DEVICE:
            self._sync_torch()
        ca = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        n = int(ca.size)
        pr = _Ref(None)
        if prior is not None:
            if _is_torch(prior):
                prior = prior.reshape(n, n).cpu() if mem == FBR_HOST else prior.reshape(n, n).to(f"cuda:{self.device}")
            else:
                prior = np.ascontiguousarray(prior, dtype=np.float64).reshape(n, n)
                if mem == FBR_DEVICE:
                    prior = torch.from_numpy(prior).to(f"cuda:{self.device}")
            pr = _Ref(prior, (n, n), "prior")
        sc = None if scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (max(C, 1),)))
        ok = C >= 1 and 1 <= n <= min(Pa, FBR_MAX_DOPT_COLUMNS)  # (else the call refuses before it touches an output: tiny stand-ins)
        tr, terms = self._out(None, (max(C, 1), 4), mem)
        er, eig = self._out(None, (C, n), mem) if eigenvalues and ok else (_Ref(None), None)
        cr, Cm = self._out(None, (C, n, n), mem) if weights and ok else (_Ref(None), None)
        if mem == FBR_DEVICE:
            status = torch.empty((max(C, 1),), dtype=torch.int32, device=f"cuda:{self.device}")  # (the kernel writes every word)
            sptr = status.data_ptr()
        else:
            status = np.zeros((max(C, 1),), dtype=np.int32)
            sptr = status.ctypes.data
        _check(self._lib.fbr_dopt_terms(self._h, Gr.ptr, C, Pa, ca.ctypes.data_as(_ip), n, pr.ptr, float(reg),
                                        None if sc is None else sc.ctypes.data_as(_dp), tr.ptr, sptr, er.ptr, cr.ptr, mem), "fbr_dopt_terms")
        out = {"neg_log_det": terms[:, 0], "lambda_max": terms[:, 1], "delta": terms[:, 2],
               "n_observable": terms[:, 3].to(torch.int64) if mem == FBR_DEVICE else terms[:, 3].astype(np.int64), "status": status}
        if eigenvalues:
            out["eig"] = eig
        if weights:
            out["Cmat"] = Cm
            st = status.cpu().numpy() if mem == FBR_DEVICE else status
            if st.any():
                err = np.linalg.LinAlgError(f"dopt_terms(weights=True): no weight matrix for candidates {np.nonzero(st)[0].tolist()} "
                                            f"(status {st[st != 0].tolist()}: 1 = a non-finite Gram, 2 = M + delta I is not positive definite)")
                err.status = st.copy()  # every candidate's status word
                raise err
        if device_out is not None and bool(device_out) != (mem == FBR_DEVICE):
            out = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(f"cuda:{self.device}") if device_out else v.cpu().numpy()) for k, v in out.items()}
        elif mem == FBR_HOST:
            out = {k: np.ascontiguousarray(v) for k, v in out.items()}
        return out

    def dopt_observability(self, G, cols, threshold: float = 1e-6, prior=None, eigenvalues: bool = False, vectors: bool = False,
                           device_out: bool | None = None) -> dict:
        """The observability analysis of C candidates from their Grams ``G`` (C, Pa, Pa) on the device (``fbr_dopt_observability``): what
        the reference runs on ``YBase`` by SVD (trajectory.py:225-264), from the eigenpairs of ``M = G[cols, cols] (+ prior)``.  Per
        candidate ``n_observable`` (int64; the eigenvalues not below ``threshold**2 * lambda_max``), ``energy`` (C, ncols) (the squared
        components of the unobservable eigenvectors per column), ``margin`` (the relative distance of the nearest eigenvalue from that
        cut) and ``status`` (int32; bit 1: a non-finite entry, the candidate's numbers are NaN; bit 4: an eigenvalue lies within the
        error band of the cut, its classification is not decided by the fp64 Gram; bit 8: the QL iteration did not converge, ``energy``
        and ``vec`` of that candidate are NaN).  ``eigenvalues``: also ``eig`` (C, ncols), bit for bit that of ``dopt_terms``;
        ``vectors``: also ``vec`` (C, ncols, ncols), ``vec[c, :, i]`` the eigenvector of ``eig[c, i]``, its largest component positive.
        A ``threshold`` outside (0, 1) or with ``threshold**2 < 8 max(128, ncols) 2**-52`` is refused.  Memory spaces: as ``dopt_terms``."""
        import torch

        Gr = _Ref(G, name="G")
        if len(Gr.obj.shape) != 3 or Gr.obj.shape[1] != Gr.obj.shape[2]:
            raise ValueError(f"G: expected (C, Pa, Pa), got {tuple(Gr.obj.shape)}")
        C, Pa = int(Gr.obj.shape[0]), int(Gr.obj.shape[1])
        mem = Gr.mem
        if mem == FBR_DEVICE:
            self._sync_torch()
        ca = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        n = int(ca.size)
        pr = _Ref(None)
        if prior is not None:
            if _is_torch(prior):
                prior = prior.reshape(n, n).cpu() if mem == FBR_HOST else prior.reshape(n, n).to(f"cuda:{self.device}")
            else:
                prior = np.ascontiguousarray(prior, dtype=np.float64).reshape(n, n)
                if mem == FBR_DEVICE:
                    prior = torch.from_numpy(prior).to(f"cuda:{self.device}")
            pr = _Ref(prior, (n, n), "prior")
        ok = C >= 1 and 1 <= n <= min(Pa, FBR_MAX_DOPT_COLUMNS)  # (else the call refuses before it touches an output: tiny stand-ins)
        Cs, ns = max(C, 1), (n if ok else 1)
        gr, energy = self._out(None, (Cs, ns), mem)
        mr, margin = self._out(None, (Cs,), mem)
        er, eig = self._out(None, (C, n), mem) if eigenvalues and ok else (_Ref(None), None)
        vr, vec = self._out(None, (C, n, n), mem) if vectors and ok else (_Ref(None), None)
        if mem == FBR_DEVICE:
            words = torch.empty((2, Cs), dtype=torch.int32, device=f"cuda:{self.device}")  # (the kernel writes every word)
            nptr, sptr = words[0].data_ptr(), words[1].data_ptr()
        else:
            words = np.zeros((2, Cs), dtype=np.int32)
            nptr, sptr = words[0].ctypes.data, words[1].ctypes.data
        _check(self._lib.fbr_dopt_observability(self._h, Gr.ptr, C, Pa, ca.ctypes.data_as(_ip), n, pr.ptr, float(threshold), nptr, gr.ptr, mr.ptr,
                                                er.ptr, vr.ptr, sptr, mem), "fbr_dopt_observability")
        out = {"n_observable": words[0].to(torch.int64) if mem == FBR_DEVICE else words[0].astype(np.int64), "energy": energy, "margin": margin,
               "status": words[1]}
        if eigenvalues:
            out["eig"] = eig
        if vectors:
            out["vec"] = vec
        if device_out is not None and bool(device_out) != (mem == FBR_DEVICE):
            out = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(f"cuda:{self.device}") if device_out else v.cpu().numpy()) for k, v in out.items()}
        elif mem == FBR_HOST:
            out = {k: np.ascontiguousarray(v) for k, v in out.items()}
        return out

    def fourier_gradient(self, wf, a, b, sens_q, sens_dq, sens_ddq, T: int, freq: float, q_range=None, tstride: int = 1, device_out: bool | None = None):
        """Chain of sensitivities (C * T, n) with the Jacobian of the series of ``fourier_states`` (``fbr_fourier_gradient``): a (C, 1 + 2 n +
        2 n nharm) array ``[wf | q_offset (n) | q_range (n) | a (n, nharm) | b (n, nharm)]``; sample i of a candidate sits at time
        ``i * tstride / freq``.  A CUDA tensor when the sensitivities are (``device_out`` overrides), else NumPy."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        C, n, nh = a.shape
        if n != self.n or b.shape != a.shape:
            raise ValueError(f"a / b: expected (C, {self.n}, nharm)")
        wf = np.ascontiguousarray(np.broadcast_to(np.asarray(wf, dtype=np.float64), (C,)))
        qr = None if q_range is None else np.ascontiguousarray(q_range, dtype=np.float64).reshape(C, n)
        refs = [_Ref(x, (C * int(T), n), nm) for x, nm in ((sens_q, "sens_q"), (sens_dq, "sens_dq"), (sens_ddq, "sens_ddq"))]
        mem = _same_space(refs)
        if mem == FBR_DEVICE:
            self._sync_torch()
        out_mem = mem if device_out is None else (FBR_DEVICE if device_out else FBR_HOST)
        r, ret = self._out(None, (C, 1 + 2 * n + 2 * n * nh), out_mem)
        _check(self._lib.fbr_fourier_gradient(self._h, C, int(T), int(tstride), nh, float(freq), wf.ctypes.data_as(_dp), a.ctypes.data_as(_dp),
                                              b.ctypes.data_as(_dp), None if qr is None else qr.ctypes.data_as(_dp), refs[0].ptr, refs[1].ptr,
                                              refs[2].ptr, mem, r.ptr, r.mem), "fbr_fourier_gradient")
        return ret

    def tsqr(self, st: dict, rhs=None, w=None, R_in=None, out=None, cols=None):
        """Upper-triangular R with R^T R = [Y[:, cols]|rhs]^T [Y[:, cols]|rhs] (blocked Householder TSQR);
        ``cols=None`` takes every identified column."""
        s, keep, S, mem = self._states(st)
        rr, wr, k = self._rhs(rhs, w, S, mem)
        ca = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
        Pa = (self.cols if ca is None else int(ca.size)) + k
        r, ret = self._out(out, (Pa, Pa), mem)
        rin = _Ref(R_in, (Pa, Pa), "R_in") if R_in is not None else _Ref(None)
        if rin.mem is not None and rin.mem != r.mem:
            raise ValueError("R_in must live in the same memory space as the output")
        if ca is None:
            _check(self._lib.fbr_tsqr(self._h, ctypes.byref(s), rr.ptr, k, wr.ptr, rin.ptr, r.ptr, r.mem), "fbr_tsqr")
        else:
            _check(self._lib.fbr_tsqr_cols(self._h, ctypes.byref(s), ca.ctypes.data_as(_ip), int(ca.size), rr.ptr, k, wr.ptr,
                                           rin.ptr, r.ptr, r.mem), "fbr_tsqr_cols")
        return ret

    def tsqr_merge(self, R_a, R_b, out=None):
        a = _Ref(R_a, name="R_a")
        n = a.obj.shape[0]
        b = _Ref(R_b, (n, n), "R_b")
        if a.mem != b.mem:
            raise ValueError("R_a and R_b must live in the same memory space")
        if a.mem == FBR_DEVICE:
            self._sync_torch()  # (a factor just received by torch.distributed lands on torch's stream)
        r, ret = self._out(out, (n, n), a.mem)
        _check(self._lib.fbr_tsqr_merge(self._h, n, a.ptr, b.ptr, r.ptr, a.mem), "fbr_tsqr_merge")
        return ret

    # ------------------------------------------------------------------ signal conditioning (Data.preprocess on the device)
    def _sig_array(self, X, ncols):
        """(pointer, mem, S, ld, keep-alive) of a 2-D C-contiguous float64 array (NumPy, changed in place, or CUDA tensor)."""
        if _is_torch(X):
            if X.dim() != 2 or not X.is_contiguous() or str(X.dtype) != "torch.float64" or X.device.type != "cuda":
                raise ValueError("expected a contiguous 2-D float64 CUDA tensor")
            self._sync_torch()
            return X.data_ptr(), FBR_DEVICE, int(X.shape[0]), int(X.shape[1]), X
        if not (isinstance(X, np.ndarray) and X.ndim == 2 and X.flags.c_contiguous and X.dtype == np.float64):
            raise ValueError("expected a C-contiguous 2-D float64 ndarray (it is filtered in place)")
        return X.ctypes.data, FBR_HOST, int(X.shape[0]), int(X.shape[1]), X

    def filtfilt(self, b, a, X, ncols=None):
        """In place ``X[:, :ncols] = scipy.signal.filtfilt(b, a, X[:, :ncols], axis=0)`` (zero-phase low-pass of every channel)."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        a = np.ascontiguousarray(a, dtype=np.float64)
        if b.size != a.size:  # scipy pads the shorter one with zeros
            n = max(b.size, a.size)
            b, a = np.r_[b, np.zeros(n - b.size)], np.r_[a, np.zeros(n - a.size)]
        ptr, mem, S, ld, keep = self._sig_array(X, ncols)
        nc = ld if ncols is None else int(ncols)
        _check(self._lib.fbr_filtfilt(self._h, b.ctypes.data_as(_dp), a.ctypes.data_as(_dp), int(b.size), ptr, S, nc, ld, mem), "fbr_filtfilt")
        return X

    def medfilt(self, k: int, X, ncols=None):
        """In place ``X[:, :ncols] = scipy.signal.medfilt(X[:, :ncols], (k, 1))``."""
        ptr, mem, S, ld, keep = self._sig_array(X, ncols)
        nc = ld if ncols is None else int(ncols)
        _check(self._lib.fbr_medfilt(self._h, int(k), ptr, S, nc, ld, mem), "fbr_medfilt")
        return X

    def central_diff(self, A, times, out=None):
        """4th-order central difference of the columns of A over the time stamps (data.py:396-418)."""
        ptr, mem, S, ld, keep = self._sig_array(A, None)
        t = _Ref(times, (S,), "times")
        if t.mem != mem:
            raise ValueError("times must live in the same memory space as A")
        r, ret = self._out(out, (S, ld), mem)
        _check(self._lib.fbr_central_diff(self._h, ptr, t.ptr, r.ptr, S, ld, mem), "fbr_central_diff")
        return ret

    def tsqr_work_info(self, num_samples: int, k: int = 0, cols=None) -> dict:
        """Executed MFMA instructions of ``tsqr(..)`` for ``num_samples`` samples (level-0 folds, merge tree), 2 * 16 * 16 * 4 = 2048 flop each."""
        ca = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
        l0, tr = ctypes.c_int64(), ctypes.c_int64()
        mb, npad = ctypes.c_int32(), ctypes.c_int32()
        _check(
            self._lib.fbr_tsqr_work_info(self._h, None if ca is None else ca.ctypes.data_as(_ip), 0 if ca is None else int(ca.size), int(k),
                                         int(num_samples), ctypes.byref(l0), ctypes.byref(tr), ctypes.byref(mb), ctypes.byref(npad)),
            "fbr_tsqr_work_info",
        )
        return {"mfma_level0": l0.value, "mfma_tree": tr.value, "block_rows": mb.value, "n_padded": npad.value,
                "flop": 2048 * (l0.value + tr.value)}

    PROF_CLASSES = ("kin", "regressor", "gram", "reduce", "id", "tsqr", "pack", "h2d", "tree")

    def profile_enable(self, on: bool = True) -> None:
        _check(self._lib.fbr_profile_enable(self._h, int(bool(on))), "fbr_profile_enable")

    def profile_get(self) -> dict:
        """{class: (device ms, launches)} since the last call (resets the counters)."""
        n = len(self.PROF_CLASSES)
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int64 * n)()
        _check(self._lib.fbr_profile_get(self._h, ms, cnt), "fbr_profile_get")
        return {c: (float(ms[i]), int(cnt[i])) for i, c in enumerate(self.PROF_CLASSES)}

    def link_merge_info(self, num_samples: int = -1) -> dict:
        """What a Gram pass over ``num_samples`` samples runs on (-1: a batch large enough for the column reductions): the moving bodies
        (links attached by fixed joints are merged into the body they ride on and the result expanded, fbr.h fbr_model_link_merge_info)."""
        ml, rc = ctypes.c_int32(), ctypes.c_int32()
        _check(self._lib.fbr_model_link_merge_info(self._h, int(num_samples), ctypes.byref(ml), ctypes.byref(rc)), "fbr_model_link_merge_info")
        return {"moving_links": ml.value, "reduced_cols": rc.value, "links": self.topo.num_links, "cols": self.cols}

    def gram_program_info(self, k: int = 0, num_samples: int = -1) -> dict:
        """Tile program ``gram(..)`` executes for a batch of ``num_samples`` samples (-1: large batches)."""
        nt, npairs, parts = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        mf = ctypes.c_int64()
        _check(
            self._lib.fbr_gram_program_info(self._h, int(k), int(num_samples), ctypes.byref(nt), ctypes.byref(npairs), ctypes.byref(mf),
                                            ctypes.byref(parts)),
            "fbr_gram_program_info",
        )
        return {"tiles": nt.value, "pairs": npairs.value, "mfma_per_sample": mf.value, "parts": parts.value}

    def gram_lane_info(self, k: int = 0, num_samples: int = -1) -> dict:
        """The sample-contiguous Gram pass (option ``gram_lane``) for such a batch; ``active`` False: the per-sample-image pass runs."""
        a = (ctypes.c_int64 * 12)()
        _check(self._lib.fbr_gram_lane_info(self._h, int(k), int(num_samples), a), "fbr_gram_lane_info")
        keys = ("active", "tile_rows", "block_image_bytes", "mfma_per_block", "levels", "max_slabs", "lds_bytes", "tiles", "force_tiles",
                "busiest_wave_pair_levels", "balanced_pair_levels", "stages")
        d = dict(zip(keys, (int(v) for v in a)))
        d["active"] = bool(d["active"])
        return d
