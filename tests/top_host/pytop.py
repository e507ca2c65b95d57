"""ctypes view of the CPU harness of the register-exchange top's plan decision (tests/top_host/harness.cpp)."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

PLAN_FIELDS = ("top_regs", "addr", "ready", "packed", "fresh", "threads", "inst_per_wg", "pcr_rows", "stages", "addr_run", "top_regs_run", "lds_bytes", "pcr_level")
DECIDE_FIELDS = ("top_regs", "stages", "top_regs_run", "shape_top_regs")


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_top_host.so")
        i64p = C.POINTER(C.c_int64)
        L.spicey_trhost_plan.restype = C.c_int32
        L.spicey_trhost_plan.argtypes = [C.POINTER(abi.SpiceyDesc), C.POINTER(abi.SpiceyOptions), C.c_int32, C.c_int64, i64p]
        L.spicey_trhost_decide.restype = None
        L.spicey_trhost_decide.argtypes = [C.c_int32, C.c_int32, C.c_int32, i64p]
        L.spicey_trhost_shapes.restype = None
        L.spicey_trhost_shapes.argtypes = [C.POINTER(C.c_int32)]
        _LIB = L
    return _LIB


def plan(flat: abi.FlatCircuit, steps: int = 64, ncu: int = 256, **options) -> dict:
    """spicey_create's plan for `flat` on a device of `ncu` CUs (environment knobs as in spicey_create), and which kernel a
    run of `steps` steps on it takes."""
    opt = abi.SpiceyOptions()
    for k, v in options.items():
        setattr(opt, k, v)
    out = np.zeros(len(PLAN_FIELDS), np.int64)
    d = flat.desc()
    rc = lib().spicey_trhost_plan(C.byref(d), C.byref(opt), ncu, steps, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"rc": rc, **dict(zip(PLAN_FIELDS, (int(x) for x in out)))}


def shapes() -> dict:
    out = np.zeros(3, np.int32)
    lib().spicey_trhost_shapes(out.ctypes.data_as(C.POINTER(C.c_int32)))
    return {"packed_fresh": int(out[0]), "packed_default": int(out[1]), "latency": int(out[2])}


def decide(addr: bool, pcr_n: int, shape: int = None) -> dict:
    """The plan's decision for a synthetic top of `pcr_n` rows (see the harness)."""
    if shape is None:
        shape = shapes()["packed_fresh"]
    out = np.zeros(len(DECIDE_FIELDS), np.int64)
    lib().spicey_trhost_decide(1 if addr else 0, pcr_n, shape, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return dict(zip(DECIDE_FIELDS, (int(x) for x in out)))
