"""ctypes view of the CPU harness of the ready-argument builds (tests/ready_host/harness.cpp)."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

RUN_FIELDS = ("nV", "nS", "pcr_n", "fresh_fill", "slots_fit", "zrec", "nOut", "nCur")
WORD_FIELDS = ("ZPAR", "SRC", "ITERS", "OUT_V", "OUT_I", "C_VPREV", "D_VDPREV", "RUN")
PLAN_FIELDS = ("ready", "slots", "early", "fresh", "packed", "threads", "lds_bytes", "ready_run")


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_ready_host.so")
        i64p = C.POINTER(C.c_int64)
        L.spicey_rahost_run.restype = C.c_int32
        L.spicey_rahost_run.argtypes = ([C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int64] + [C.c_void_p] * 8
                                        + [C.c_int32, C.c_void_p, i64p])
        L.spicey_rahost_words.restype = None
        L.spicey_rahost_words.argtypes = [C.POINTER(C.c_int32)]
        L.spicey_rahost_plan.restype = C.c_int32
        L.spicey_rahost_plan.argtypes = [C.POINTER(abi.SpiceyDesc), C.POINTER(abi.SpiceyOptions), C.c_int32, C.c_int64, i64p]
        _LIB = L
    return _LIB


def words() -> dict:
    """Index of the table's words by name."""
    out = np.zeros(8, np.int32)
    lib().spicey_rahost_words(out.ctypes.data_as(C.POINTER(C.c_int32)))
    return dict(zip(WORD_FIELDS, (int(x) for x in out)))


def run(flat: abi.FlatCircuit, steps: int, dt: float, src, ready: bool, T: int = 512, reverse: bool = False, nan_fill: bool = False, currents: bool = True) -> dict:
    """One emulated run at the packed layout (T threads, 4 slots) of the fresh-fill program on the operand-slot build.
    src: (steps + 1, nV) for every instance, or (n_inst, steps + 1, nV).  The result keeps the buffers alive whose addresses
    the table's words are made of ("addr")."""
    ni = flat.n_inst
    src = np.ascontiguousarray(src, dtype=np.float64)
    stride = 0 if src.ndim < 3 else int(src[0].size)
    out_v = np.zeros((ni, steps + 1, flat.n_out))
    out_i = np.zeros((ni, steps + 1, flat.n_cur)) if currents else None
    iters = np.zeros((ni, steps + 1), np.int32)
    zpar = np.full(ni * 2 * T * 5, np.nan if nan_fill else 0.0)
    st = {"C_vprev": flat.C_vprev.copy(), "L_iprev": flat.L_iprev.copy(), "D_vdprev": flat.D_vdprev.copy(), "S_ison": flat.S_ison.copy()}
    info = np.zeros(8, np.int64)
    table = np.zeros((ni, words()["RUN"]), np.uint32)
    d = flat.desc()
    rc = lib().spicey_rahost_run(C.byref(d), 1 if ready else 0, T, steps, dt, src.ctypes.data, stride, zpar.ctypes.data, out_v.ctypes.data,
                                 out_i.ctypes.data if currents else None, iters.ctypes.data, st["C_vprev"].ctypes.data, st["L_iprev"].ctypes.data,
                                 st["D_vdprev"].ctypes.data, st["S_ison"].ctypes.data, (1 if reverse else 0) | (2 if nan_fill else 0), table.ctypes.data,
                                 info.ctypes.data_as(C.POINTER(C.c_int64)))
    addr = {"zpar": zpar.ctypes.data, "src": src.ctypes.data, "iters": iters.ctypes.data, "out_v": out_v.ctypes.data,
            "out_i": out_i.ctypes.data if currents else 0, "C_vprev": st["C_vprev"].ctypes.data, "D_vdprev": st["D_vdprev"].ctypes.data}
    return {"status": rc, "out_v": out_v, "out_i": out_i, "iters": iters, "state": st, "table": table, "addr": addr, "src_stride": stride,
            "keep": (zpar, src), **dict(zip(RUN_FIELDS, (int(x) for x in info)))}


def plan(flat: abi.FlatCircuit, steps: int = 64, ncu: int = 256, **options) -> dict:
    """spicey_create's plan for `flat` on a device of `ncu` CUs (environment knobs as in spicey_create), and whether a run of
    `steps` steps on it takes the ready-argument kernel."""
    opt = abi.SpiceyOptions()
    for k, v in options.items():
        setattr(opt, k, v)
    out = np.zeros(8, np.int64)
    d = flat.desc()
    rc = lib().spicey_rahost_plan(C.byref(d), C.byref(opt), ncu, steps, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"rc": rc, **dict(zip(PLAN_FIELDS, (int(x) for x in out)))}
