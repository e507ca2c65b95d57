"""ctypes view of the CPU harness of the operand-address builds (tests/addr_host/harness.cpp)."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

RUN_FIELDS = ("nV", "nS", "pcr_n", "fresh_fill", "slots_fit", "addr_fits", "nW", "nU", "nGdyn", "slot_index", "nOut", "nCur", "n", "nKeep", "max_index",
              "arena_doubles")
REG_FIELDS = ("dd0", "dd1", "rhs00", "rhs01", "rhs10", "rhs11", "eR0", "eR1", "eC0", "eC1", "eD0", "eD1", "ox0", "ox1")
RAW_FIELDS = ("dd0", "dd1", "rhs00", "rhs01", "rhs10", "rhs11")
PLAN_FIELDS = ("addr", "ready", "slots", "early", "fresh", "packed", "threads", "lds_bytes", "ready_run", "addr_run", "info_operand_addr", "inst_per_wg")
FIT_FIELDS = ("slots_fit", "addr_fits", "max_index", "field_max", "plan_addr", "ready_run", "addr_run", "shape_addr")


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_addr_host.so")
        i64p = C.POINTER(C.c_int64)
        L.spicey_oahost_run.restype = C.c_int32
        L.spicey_oahost_run.argtypes = ([C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int64] + [C.c_void_p] * 8
                                        + [C.c_int32, C.c_void_p, C.c_void_p, i64p])
        L.spicey_oahost_plan.restype = C.c_int32
        L.spicey_oahost_plan.argtypes = [C.POINTER(abi.SpiceyDesc), C.POINTER(abi.SpiceyOptions), C.c_int32, C.c_int64, i64p]
        L.spicey_oahost_fits.restype = None
        L.spicey_oahost_fits.argtypes = [C.c_int32] * 10 + [i64p]
        L.spicey_oahost_shapes.restype = None
        L.spicey_oahost_shapes.argtypes = [C.POINTER(C.c_int32)]
        _LIB = L
    return _LIB


def run(flat: abi.FlatCircuit, steps: int, dt: float, src, addr: bool, T: int = 512, reverse: bool = False, nan_fill: bool = False, currents: bool = True) -> dict:
    """One emulated run at the packed layout (T threads, 4 slots) of the fresh-fill program on the ready-argument build,
    with operand addresses or without.  src: (steps + 1, nV) for every instance, or (n_inst, steps + 1, nV).  "regs": per
    instance and thread the descriptor and terminal registers after the run (REG_FIELDS); "raw": per thread the program's
    own descriptors of the same items (RAW_FIELDS)."""
    ni = flat.n_inst
    src = np.ascontiguousarray(src, dtype=np.float64)
    stride = 0 if src.ndim < 3 else int(src[0].size)
    out_v = np.zeros((ni, steps + 1, flat.n_out))
    out_i = np.zeros((ni, steps + 1, flat.n_cur)) if currents else None
    iters = np.zeros((ni, steps + 1), np.int32)
    zpar = np.full(ni * 2 * T * 5, np.nan if nan_fill else 0.0)
    st = {"C_vprev": flat.C_vprev.copy(), "L_iprev": flat.L_iprev.copy(), "D_vdprev": flat.D_vdprev.copy(), "S_ison": flat.S_ison.copy()}
    info = np.zeros(16, np.int64)
    regs = np.zeros((ni, T, len(REG_FIELDS)), np.uint32)
    raw = np.zeros((T, len(RAW_FIELDS)), np.uint32)
    d = flat.desc()
    rc = lib().spicey_oahost_run(C.byref(d), 1 if addr else 0, T, steps, dt, src.ctypes.data, stride, zpar.ctypes.data, out_v.ctypes.data,
                                 out_i.ctypes.data if currents else None, iters.ctypes.data, st["C_vprev"].ctypes.data, st["L_iprev"].ctypes.data,
                                 st["D_vdprev"].ctypes.data, st["S_ison"].ctypes.data, (1 if reverse else 0) | (2 if nan_fill else 0), regs.ctypes.data,
                                 raw.ctypes.data, info.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"status": rc, "out_v": out_v, "out_i": out_i, "iters": iters, "state": st, "regs": regs, "raw": raw,
            **dict(zip(RUN_FIELDS, (int(x) for x in info)))}


def plan(flat: abi.FlatCircuit, steps: int = 64, ncu: int = 256, **options) -> dict:
    """spicey_create's plan for `flat` on a device of `ncu` CUs (environment knobs as in spicey_create), and which kernel a
    run of `steps` steps on it takes."""
    opt = abi.SpiceyOptions()
    for k, v in options.items():
        setattr(opt, k, v)
    out = np.zeros(len(PLAN_FIELDS), np.int64)
    d = flat.desc()
    rc = lib().spicey_oahost_plan(C.byref(d), C.byref(opt), ncu, steps, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"rc": rc, **dict(zip(PLAN_FIELDS, (int(x) for x in out)))}


def shapes() -> dict:
    out = np.zeros(3, np.int32)
    lib().spicey_oahost_shapes(out.ctypes.data_as(C.POINTER(C.c_int32)))
    return {"packed_fresh": int(out[0]), "hybrid": int(out[1]), "packed_default": int(out[2])}


def fits(nW: int, nU: int, nGdyn: int, nS: int = 0, pcr_n: int = 64, pcr_level: int = 2, tail_n: int = 0, hybrid: int = 0, K: int = 1, shape: int = None) -> dict:
    """The fit rule and the plan's decision for a synthetic program header (see the harness)."""
    if shape is None:
        shape = shapes()["packed_fresh"]
    out = np.zeros(len(FIT_FIELDS), np.int64)
    lib().spicey_oahost_fits(nW, nU, nGdyn, nS, pcr_n, pcr_level, tail_n, hybrid, K, shape, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return dict(zip(FIT_FIELDS, (int(x) for x in out)))
