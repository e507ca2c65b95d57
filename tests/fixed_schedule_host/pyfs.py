"""ctypes view of the CPU harness of the fixed schedule (tests/fixed_schedule_host/harness.cpp)."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

INFO_FIELDS = ("fs_fits", "fuse_ok", "fold_ok", "n_levels", "pcr_level", "k_merge", "streamed_phases", "pcr_n")
PLAN_FIELDS = ("fixed_schedule", "stamp_fuse", "top_fold", "packed", "fresh", "threads", "fixed_schedule_run", "stamp_fuse_run")
PREDICATE_FIELDS = ("as_built", "streamed_backward_phase", "unmerged", "three_products", "empty_factor_phase", "lds_tail", "top_of_65_rows")


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_fixed_schedule_host.so")
        i64p = C.POINTER(C.c_int64)
        L.spicey_fshost_run.restype = C.c_int32
        L.spicey_fshost_run.argtypes = ([C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int64] + [C.c_void_p] * 7
                                        + [C.c_int32, i64p, C.c_void_p, i64p])
        L.spicey_fshost_plan.restype = C.c_int32
        L.spicey_fshost_plan.argtypes = [C.POINTER(abi.SpiceyDesc), C.POINTER(abi.SpiceyOptions), C.c_int32, C.c_int64, i64p]
        L.spicey_fshost_predicate.restype = C.c_int32
        L.spicey_fshost_predicate.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, i64p]
        _LIB = L
    return _LIB


def run(flat: abi.FlatCircuit, steps: int, dt: float, src, fixed: bool, T: int = 512, reverse: bool = False, nan_fill: bool = False, currents: bool = True,
        state: dict = None, idle_waves: bool = True, iters_fill: int = 0) -> dict:
    """One emulated run at the packed layout (T threads, 4 slots) of the fresh-fill program on the operand-address build in its
    fused form, or (fixed) in that form's fixed schedule.  src: (steps + 1, nV) for every instance, or (n_inst, steps + 1, nV).
    state: the end state of an earlier run to start from (default: the circuit's).  iters_fill: what the iteration counts hold
    before the run."""
    ni = flat.n_inst
    src = np.ascontiguousarray(src, dtype=np.float64)
    stride = 0 if src.ndim < 3 else int(src[0].size)
    out_v = np.zeros((ni, steps + 1, flat.n_out))
    out_i = np.zeros((ni, steps + 1, flat.n_cur)) if currents else None
    iters = np.full((ni, steps + 1), iters_fill, np.int32)
    st = {k: np.array(v, copy=True) for k, v in (state or {"C_vprev": flat.C_vprev, "L_iprev": flat.L_iprev, "D_vdprev": flat.D_vdprev, "S_ison": flat.S_ison}).items()}
    info = np.zeros(len(INFO_FIELDS), np.int64)
    err4 = np.zeros(4, np.int32)
    solves = np.zeros(1, np.int64)
    d = flat.desc()
    rc = lib().spicey_fshost_run(C.byref(d), 1 if fixed else 0, T, steps, dt, src.ctypes.data, stride, out_v.ctypes.data, out_i.ctypes.data if currents else None,
                                 iters.ctypes.data, st["C_vprev"].ctypes.data, st["L_iprev"].ctypes.data, st["D_vdprev"].ctypes.data, st["S_ison"].ctypes.data,
                                 (1 if reverse else 0) | (2 if nan_fill else 0) | (0 if idle_waves else 4), info.ctypes.data_as(C.POINTER(C.c_int64)), err4.ctypes.data,
                                 solves.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"status": rc, "out_v": out_v, "out_i": out_i, "iters": iters, "state": st, "err4": err4, "solves": int(solves[0]),
            **dict(zip(INFO_FIELDS, (int(x) for x in info)))}


def plan(flat: abi.FlatCircuit, steps: int = 64, ncu: int = 256, **options) -> dict:
    """spicey_create's plan for `flat` on a device of `ncu` CUs (environment knobs as in spicey_create), and which kernel a
    run of `steps` steps on it takes."""
    opt = abi.SpiceyOptions()
    for k, v in options.items():
        setattr(opt, k, v)
    out = np.zeros(len(PLAN_FIELDS), np.int64)
    d = flat.desc()
    rc = lib().spicey_fshost_plan(C.byref(d), C.byref(opt), ncu, steps, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"rc": rc, **dict(zip(PLAN_FIELDS, (int(x) for x in out)))}


def predicate(flat: abi.FlatCircuit, T: int = 512) -> dict:
    """spicey_fixed_schedule_fits on the packed layout of `flat` as built, and on that layout with one condition broken at a time."""
    out = np.zeros(8, np.int64)
    d = flat.desc()
    rc = lib().spicey_fshost_predicate(C.byref(d), T, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"rc": rc, **dict(zip(PREDICATE_FIELDS, (int(x) for x in out)))}
