"""ctypes view of the CPU harness of the stamp fuse (tests/stamp_fuse_host/harness.cpp)."""
import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

INFO_FIELDS = ("table_ok", "fold_ok", "u0_fits", "n_keep", "n", "n_dyn_ent", "n_v", "xoff")
PLAN_FIELDS = ("stamp_fuse", "top_fold", "packed", "fresh", "threads", "stamp_fuse_run", "top_fold_run", "zpar_doubles")
TABLE_FIELDS = ("n_keep", "n", "n_dyn_ent", "n_v", "xoff", "n_c", "n_d", "fold_ok")

# a slot word (spicey_amd/csrc/tran_pt_layout.h: SPICEY_SF_*)
NONE, RECIP, F0, F0_NEG, F1, F1_NEG, SWAP = 0x80000000, 0x40000000, 0x10000, 0x20000, 0x40000, 0x80000, 0x100000


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_stamp_fuse_host.so")
        i64p = C.POINTER(C.c_int64)
        L.spicey_sfhost_run.restype = C.c_int32
        L.spicey_sfhost_run.argtypes = ([C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_int64] + [C.c_void_p] * 7
                                        + [C.c_int32, i64p, C.c_void_p, i64p])
        L.spicey_sfhost_plan.restype = C.c_int32
        L.spicey_sfhost_plan.argtypes = [C.POINTER(abi.SpiceyDesc), C.POINTER(abi.SpiceyOptions), C.c_int32, C.c_int64, i64p]
        L.spicey_sfhost_table.restype = C.c_int32
        L.spicey_sfhost_table.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i64p]
        _LIB = L
    return _LIB


def run(flat: abi.FlatCircuit, steps: int, dt: float, src, fuse: bool, T: int = 512, reverse: bool = False, nan_fill: bool = False, currents: bool = True,
        state: dict = None) -> dict:
    """One emulated run at the packed layout (T threads, 4 slots) of the fresh-fill program on the operand-address build: the
    form a plan without the fuse takes (the folded top where it fits), or the fuse on top of the fold.  src: (steps + 1, nV)
    for every instance, or (n_inst, steps + 1, nV).  state: the end state of an earlier run to start from (default: the
    circuit's)."""
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
    rc = lib().spicey_sfhost_run(C.byref(d), 1 if fuse else 0, T, steps, dt, src.ctypes.data, stride, out_v.ctypes.data, out_i.ctypes.data if currents else None,
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
    rc = lib().spicey_sfhost_plan(C.byref(d), C.byref(opt), ncu, steps, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return {"rc": rc, **dict(zip(PLAN_FIELDS, (int(x) for x in out)))}


def table(flat: abi.FlatCircuit, T: int = 512) -> dict:
    """The fuse's table of `flat` as (T, 6) words — columns 0, 1: entry slots, 2, 3: row slots, 4: the source's row —, and what it was dealt
    from: the descriptors of the stamped entries, of the rows (n, 2), and the sources' branch-current indices."""
    tb = np.zeros(6 * T, np.uint32)
    dd = np.zeros(2 * T, np.uint32)
    rows = np.zeros(4 * T, np.uint32)
    vx = np.zeros(T, np.int32)
    info = np.zeros(8, np.int64)
    d = flat.desc()
    ok = lib().spicey_sfhost_table(C.byref(d), T, tb.ctypes.data, dd.ctypes.data, rows.ctypes.data, vx.ctypes.data, info.ctypes.data_as(C.POINTER(C.c_int64)))
    f = dict(zip(TABLE_FIELDS, (int(x) for x in info)))
    return {"ok": ok, "table": tb.reshape(T, 6), "ent_dd": dd[:min(f["n_keep"], 2 * T)], "row_desc": rows.reshape(2 * T, 2)[:min(f["n"], 2 * T)], "V_x": vx[:min(f["n_v"], T)], **f}
