"""ctypes front-end of tests/exact_host/harness.cpp: the reference-order engine (spicey_amd/csrc/exact_exec.h) run on the
CPU through the product's own plan and stamp lists (test infrastructure)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import harness_build
from spicey_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(_HERE, "libspicey_exact_host.so")
        f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        L.spicey_exact_host_run.restype = C.c_int32
        L.spicey_exact_host_run.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_double, f64p, f64p, f64p,
                                            i32p, f64p, f64p, f64p, i32p, i64p, f64p, i32p, C.POINTER(abi.SpiceyInfo)]
        L.spicey_exact_host_lists.restype = C.c_int32
        L.spicey_exact_host_lists.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, i32p, i32p, C.c_int32, i32p, i32p]
        _LIB = L
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


class ExactHostBackend:
    """Same `run` interface as spicey_amd.lib.HipBackend.  T = threads of the emulated workgroup (0 = the plan's choice),
    global_ws = the global-slab layout, reverse = every phase's threads in reverse order.  The state carried between two
    runs is the caller's (simulateTRAN writes it back to the circuit)."""

    def __init__(self, T: int = 0, global_ws: bool = False, reverse: bool = False):
        self.T, self.global_ws, self.reverse = T, global_ws, reverse
        self.info = None

    def run(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, want_currents: bool = True,
            want_iters: bool = True) -> dict:
        L = lib()
        d = flat.desc()
        ni = flat.n_inst
        src = np.ascontiguousarray(src, dtype=np.float64)
        out_v = np.zeros((ni, steps + 1, flat.n_out))
        out_i = np.zeros((ni, steps + 1, flat.n_cur)) if want_currents else None
        iters = np.zeros((ni, steps + 1), np.int32) if want_iters else None
        st = {"C_vprev": flat.C_vprev.copy(), "L_iprev": flat.L_iprev.copy(), "D_vdprev": flat.D_vdprev.copy(),
              "S_ison": flat.S_ison.copy()}
        skip = np.zeros(ni, np.int64)
        lin_err = np.zeros((ni, steps + 1))
        err4 = np.zeros(4, np.int32)
        info = abi.SpiceyInfo()
        rc = L.spicey_exact_host_run(C.byref(d), self.T, int(self.global_ws), int(self.reverse), steps, dt, _p(src, C.c_double),
                                     _p(out_v, C.c_double), _p(out_i, C.c_double), _p(iters, C.c_int32), _p(st["C_vprev"], C.c_double),
                                     _p(st["L_iprev"], C.c_double), _p(st["D_vdprev"], C.c_double), _p(st["S_ison"], C.c_int32),
                                     _p(skip, C.c_int64), _p(lin_err, C.c_double), _p(err4, C.c_int32), C.byref(info))
        self.info = info.as_dict()
        detail = f"singular at inst {err4[1]} step {err4[2]} iter {err4[3]}" if rc == abi.ERR_SINGULAR else ""
        return {"status": rc, "detail": detail, "out_v": out_v, "out_i": out_i, "iters": iters, "state": st,
                "skip_risk": skip, "lin_err": lin_err}


def stamp_lists(flat: abi.FlatCircuit):
    """[((row, column), [(kind, elem, which, sub), ...]), ...] in the order the engine stores them (row-major)."""
    L = lib()
    d = flat.desc()
    nt = C.c_int32(0)
    ne = L.spicey_exact_host_lists(C.byref(d), 0, None, None, 0, None, C.byref(nt))
    assert ne >= 0
    rc = np.zeros((max(ne, 1), 2), np.int32)
    ptr = np.zeros(ne + 1, np.int32)
    terms = np.zeros((max(nt.value, 1), 4), np.int32)
    assert L.spicey_exact_host_lists(C.byref(d), ne, _p(rc, C.c_int32), _p(ptr, C.c_int32), nt.value, _p(terms, C.c_int32), C.byref(nt)) == ne
    kinds = "RCLSVD"
    return [((int(rc[e, 0]), int(rc[e, 1])), [(kinds[t[0]], int(t[1]), int(t[2]), int(t[3])) for t in terms[ptr[e]:ptr[e + 1]]])
            for e in range(ne)]
