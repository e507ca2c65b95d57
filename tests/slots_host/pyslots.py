"""ctypes view of the CPU harness of the operand-slot builds (tests/slots_host/harness.cpp)."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

RUN_FIELDS = ("nV", "nS", "pcr_n", "fresh_fill", "slots_fit", "slot_index", "bits_plus", "bits_minus")
WHERE_FIELDS = ("fit", "slot_index", "end_bytes", "lds_bytes")
PLAN_FIELDS = ("slots", "early", "fresh", "packed", "threads", "lds_bytes")


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_slots_host.so")
        i64p = C.POINTER(C.c_int64)
        L.spicey_slots_run.restype = C.c_int32
        L.spicey_slots_run.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int64, C.c_double] + [C.c_void_p] * 8 + [C.c_int32, i64p]
        L.spicey_slots_where.restype = None
        L.spicey_slots_where.argtypes = [C.c_int32] * 7 + [i64p]
        L.spicey_slots_plan.restype = C.c_int32
        L.spicey_slots_plan.argtypes = [C.POINTER(abi.SpiceyDesc), C.POINTER(abi.SpiceyOptions), C.c_int32, i64p]
        _LIB = L
    return _LIB


def run(flat: abi.FlatCircuit, steps: int, dt: float, src, slots: bool, T: int = 512, reverse: bool = False, nan_fill: bool = False) -> dict:
    """One emulated run at the packed layout (T threads, 4 slots) of the fresh-fill program on the early-prefetch build."""
    ni = flat.n_inst
    src = np.ascontiguousarray(src, dtype=np.float64)
    out_v = np.zeros((ni, steps + 1, flat.n_out))
    out_i = np.zeros((ni, steps + 1, flat.n_cur))
    iters = np.zeros((ni, steps + 1), np.int32)
    st = {"C_vprev": flat.C_vprev.copy(), "L_iprev": flat.L_iprev.copy(), "D_vdprev": flat.D_vdprev.copy(), "S_ison": flat.S_ison.copy()}
    info = np.zeros(8, np.int64)
    d = flat.desc()
    rc = lib().spicey_slots_run(C.byref(d), 1 if slots else 0, T, steps, dt, src.ctypes.data, out_v.ctypes.data, out_i.ctypes.data, iters.ctypes.data,
                                st["C_vprev"].ctypes.data, st["L_iprev"].ctypes.data, st["D_vdprev"].ctypes.data, st["S_ison"].ctypes.data,
                                (1 if reverse else 0) | (2 if nan_fill else 0), info.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"status": rc, "out_v": out_v, "out_i": out_i, "iters": iters, "state": st, **dict(zip(RUN_FIELDS, (int(x) for x in info)))}


def where(nW: int, nU: int, nGdyn: int, nS: int, pcr_n: int, pcr_level: int, tail_n: int = 0) -> dict:
    """Slot positions for a program header with these fields."""
    out = np.zeros(4, np.int64)
    lib().spicey_slots_where(nW, nU, nGdyn, nS, pcr_n, pcr_level, tail_n, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return dict(zip(WHERE_FIELDS, (int(x) for x in out)))


def plan(flat: abi.FlatCircuit, ncu: int = 256, **options) -> dict:
    """spicey_create's plan for `flat` on a device of `ncu` CUs (environment knobs as in spicey_create)."""
    opt = abi.SpiceyOptions()
    for k, v in options.items():
        setattr(opt, k, v)
    out = np.zeros(6, np.int64)
    d = flat.desc()
    rc = lib().spicey_slots_plan(C.byref(d), C.byref(opt), ncu, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"rc": rc, **dict(zip(PLAN_FIELDS, (int(x) for x in out)))}
