"""ctypes view of the CPU harness of the fold of the last factor level into the top (tests/top_fold_host/harness.cpp)."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

INFO_FIELDS = ("pcr_n", "pcr_level", "n_levels", "row_records", "remainder", "table_ok", "u0_fits", "with_pivot")
PLAN_FIELDS = ("top_fold", "u0_resident", "top_regs", "addr", "packed", "fresh", "threads", "inst_per_wg", "top_fold_run", "u0_resident_run", "pcr_n", "pcr_level")


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_top_fold_host.so")
        i64p = C.POINTER(C.c_int64)
        L.spicey_tfhost_run.restype = C.c_int32
        L.spicey_tfhost_run.argtypes = ([C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int64] + [C.c_void_p] * 7
                                        + [C.c_int32, i64p, C.c_void_p, i64p])
        L.spicey_tfhost_plan.restype = C.c_int32
        L.spicey_tfhost_plan.argtypes = [C.POINTER(abi.SpiceyDesc), C.POINTER(abi.SpiceyOptions), C.c_int32, C.c_int64, i64p]
        L.spicey_tfhost_table.restype = C.c_int32
        L.spicey_tfhost_table.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, i64p]
        _LIB = L
    return _LIB


def run(flat: abi.FlatCircuit, steps: int, dt: float, src, fold: bool, T: int = 512, reverse: bool = False, nan_fill: bool = False, currents: bool = True,
        state: dict = None) -> dict:
    """One emulated run at the packed layout (T threads, 4 slots) of the fresh-fill program on the operand-address build with
    the register-exchange-top flag: the form a plan without the fold takes, or the fold.  src: (steps + 1, nV) for every
    instance, or (n_inst, steps + 1, nV).  state: the end state of an earlier run to start from (default: the circuit's)."""
    ni = flat.n_inst
    src = np.ascontiguousarray(src, dtype=np.float64)
    stride = 0 if src.ndim < 3 else int(src[0].size)
    out_v = np.zeros((ni, steps + 1, flat.n_out))
    out_i = np.zeros((ni, steps + 1, flat.n_cur)) if currents else None
    iters = np.zeros((ni, steps + 1), np.int32)
    st = {k: np.array(v, copy=True) for k, v in (state or {"C_vprev": flat.C_vprev, "L_iprev": flat.L_iprev, "D_vdprev": flat.D_vdprev, "S_ison": flat.S_ison}).items()}
    info = np.zeros(len(INFO_FIELDS), np.int64)
    err4 = np.zeros(4, np.int32)
    solves = np.zeros(1, np.int64)
    d = flat.desc()
    rc = lib().spicey_tfhost_run(C.byref(d), 1 if fold else 0, T, steps, dt, src.ctypes.data, stride, out_v.ctypes.data, out_i.ctypes.data if currents else None,
                                 iters.ctypes.data, st["C_vprev"].ctypes.data, st["L_iprev"].ctypes.data, st["D_vdprev"].ctypes.data, st["S_ison"].ctypes.data,
                                 (1 if reverse else 0) | (2 if nan_fill else 0), info.ctypes.data_as(C.POINTER(C.c_int64)), err4.ctypes.data,
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
    rc = lib().spicey_tfhost_plan(C.byref(d), C.byref(opt), ncu, steps, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"rc": rc, **dict(zip(PLAN_FIELDS, (int(x) for x in out)))}


def table(flat: abi.FlatCircuit, T: int = 512) -> dict:
    """The fold's table of `flat` (64 records of 16 half-words), the top's index table (64 x 4), the program's row records of
    the level below the top (64 x 16 half-words, program order) and the +0.0 slot's index."""
    tb = np.zeros(512, np.uint32)
    tab = np.zeros((64, 4), np.uint16)
    rows = np.zeros(512, np.uint32)
    info = np.zeros(8, np.int64)
    d = flat.desc()
    ok = lib().spicey_tfhost_table(C.byref(d), T, tb.ctypes.data, tab.ctypes.data, rows.ctypes.data, info.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"ok": ok, "table": tb.view(np.uint16).reshape(64, 16), "tab": tab, "rows": rows.view(np.uint16).reshape(64, 16), "zero_slot": int(info[7]),
            **dict(zip(INFO_FIELDS[:7], (int(x) for x in info[:7])))}
