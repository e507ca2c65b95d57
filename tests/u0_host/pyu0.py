"""ctypes view of the CPU harness of the resident level-0 record (tests/u0_host/harness.cpp)."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

RUN_FIELDS = ("rows", "records", "remainder", "fits", "pcr_n", "pcr_level", "n_levels", "addr_fits")
PLAN_FIELDS = ("u0_resident", "top_regs", "addr", "packed", "fresh", "threads", "inst_per_wg", "top_regs_run", "u0_resident_run", "rows", "records", "remainder")
DECIDE_FIELDS = ("fits", "u0_resident", "u0_resident_run", "shape_u0_resident")


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_u0_host.so")
        i64p = C.POINTER(C.c_int64)
        L.spicey_u0host_run.restype = C.c_int32
        L.spicey_u0host_run.argtypes = ([C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int64] + [C.c_void_p] * 8
                                        + [C.c_int32, C.c_void_p, C.c_void_p, i64p, C.c_void_p, i64p])
        L.spicey_u0host_plan.restype = C.c_int32
        L.spicey_u0host_plan.argtypes = [C.POINTER(abi.SpiceyDesc), C.POINTER(abi.SpiceyOptions), C.c_int32, C.c_int64, i64p]
        L.spicey_u0host_decide.restype = None
        L.spicey_u0host_decide.argtypes = [C.c_int32] * 7 + [i64p]
        L.spicey_u0host_shapes.restype = None
        L.spicey_u0host_shapes.argtypes = [C.POINTER(C.c_int32)]
        L.spicey_u0host_exp.restype = None
        L.spicey_u0host_exp.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


def run(flat: abi.FlatCircuit, steps: int, dt: float, src, resident: bool, T: int = 512, reverse: bool = False, nan_fill: bool = False, currents: bool = True,
        state: dict = None) -> dict:
    """One emulated run at the packed layout (T threads, 4 slots) of the fresh-fill program on the operand-address build with
    the register-exchange-top flag, with the resident level-0 record or without.  src: (steps + 1, nV) for every instance,
    or (n_inst, steps + 1, nV).  state: the end state of an earlier run to start from (default: the circuit's own).
    "u0": per instance and thread the eight record words after the run; "raw": per thread the program's own row record."""
    ni = flat.n_inst
    src = np.ascontiguousarray(src, dtype=np.float64)
    stride = 0 if src.ndim < 3 else int(src[0].size)
    out_v = np.zeros((ni, steps + 1, flat.n_out))
    out_i = np.zeros((ni, steps + 1, flat.n_cur)) if currents else None
    iters = np.zeros((ni, steps + 1), np.int32)
    zpar = np.full(ni * 2 * T * 5, np.nan if nan_fill else 0.0)
    st = {k: np.array(v, copy=True) for k, v in (state or {"C_vprev": flat.C_vprev, "L_iprev": flat.L_iprev, "D_vdprev": flat.D_vdprev, "S_ison": flat.S_ison}).items()}
    info = np.zeros(len(RUN_FIELDS), np.int64)
    u0 = np.zeros((ni, T, 8), np.uint32)
    raw = np.zeros((T, 8), np.uint32)
    err4 = np.zeros(4, np.int32)
    solves = np.zeros(1, np.int64)
    d = flat.desc()
    rc = lib().spicey_u0host_run(C.byref(d), 1 if resident else 0, T, steps, dt, src.ctypes.data, stride, zpar.ctypes.data, out_v.ctypes.data,
                                 out_i.ctypes.data if currents else None, iters.ctypes.data, st["C_vprev"].ctypes.data, st["L_iprev"].ctypes.data,
                                 st["D_vdprev"].ctypes.data, st["S_ison"].ctypes.data, (1 if reverse else 0) | (2 if nan_fill else 0), u0.ctypes.data,
                                 raw.ctypes.data, info.ctypes.data_as(C.POINTER(C.c_int64)), err4.ctypes.data, solves.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"status": rc, "out_v": out_v, "out_i": out_i, "iters": iters, "state": st, "u0": u0, "raw": raw, "err4": err4, "solves": int(solves[0]),
            **dict(zip(RUN_FIELDS, (int(x) for x in info)))}


def plan(flat: abi.FlatCircuit, steps: int = 64, ncu: int = 256, **options) -> dict:
    """spicey_create's plan for `flat` on a device of `ncu` CUs (environment knobs as in spicey_create), and which kernel a
    run of `steps` steps on it takes."""
    opt = abi.SpiceyOptions()
    for k, v in options.items():
        setattr(opt, k, v)
    out = np.zeros(len(PLAN_FIELDS), np.int64)
    d = flat.desc()
    rc = lib().spicey_u0host_plan(C.byref(d), C.byref(opt), ncu, steps, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"rc": rc, **dict(zip(PLAN_FIELDS, (int(x) for x in out)))}


def shapes() -> dict:
    out = np.zeros(3, np.int32)
    lib().spicey_u0host_shapes(out.ctypes.data_as(C.POINTER(C.c_int32)))
    return {"packed_fresh": int(out[0]), "packed_default": int(out[1]), "latency": int(out[2])}


def decide(rows: int, cnt: int, rcnt: int = 0, nD: int = 1, T: int = 512, top_regs: bool = True, shape: int = None) -> dict:
    """The plan's decision for a synthetic phase-0 descriptor (see the harness)."""
    if shape is None:
        shape = shapes()["packed_fresh"]
    out = np.zeros(len(DECIDE_FIELDS), np.int64)
    lib().spicey_u0host_decide(1 if top_regs else 0, rows, cnt, rcnt, nD, T, shape, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return dict(zip(DECIDE_FIELDS, (int(x) for x in out)))


def exp_pair(x) -> tuple:
    """(the port of the device library's exp as the host compiles it, the host's exp) on the doubles `x`."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    port, libm = np.empty_like(x), np.empty_like(x)
    lib().spicey_u0host_exp(x.ctypes.data, x.size, port.ctypes.data, libm.ctypes.data)
    return port, libm
