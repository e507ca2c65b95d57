"""ctypes front-end of tests/ac_exact_host/harness.cpp: the reference-order AC engine (spicey_amd/csrc/ac_exact_exec.h) run
on the CPU through the product's own plan and stamp lists (test infrastructure)."""
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
        L = harness_build.load(_HERE, "libspicey_ac_exact_host.so")
        f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        L.spicey_ac_exact_host_run.restype = C.c_int32
        L.spicey_ac_exact_host_run.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int32, C.c_int64, f64p, f64p, f64p, f64p,
                                               i32p, i64p, i64p]
        L.spicey_ac_exact_host_plan.restype = C.c_int32
        L.spicey_ac_exact_host_plan.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, C.c_int32, C.c_int64, i64p, C.c_char_p, C.c_int32]
        L.spicey_ac_exact_host_lists.restype = C.c_int32
        L.spicey_ac_exact_host_lists.argtypes = [C.POINTER(abi.SpiceyDesc), C.c_int32, i32p, i32p, C.c_int32, i32p, i32p]
        L.spicey_ac_exact_host_hypot.restype = None
        L.spicey_ac_exact_host_hypot.argtypes = [C.c_int64, f64p, f64p]
        _LIB = L
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


class AcExactHostBackend:
    """Same `run_ac` interface as spicey_amd.lib.HipBackend.  T = threads of the emulated workgroup (0 = the plan's
    choice), global_ws = the global-slab layout, reverse = every phase's threads in reverse order.  The result also
    carries the per-slot status and skip counts."""

    exact_order = True  # (simulateAC: the inductors' divide errors come from the engine, as with HipAcExactBackend)

    def __init__(self, T: int = 0, global_ws: bool = False, reverse: bool = False):
        self.T, self.global_ws, self.reverse = T, global_ws, reverse

    def run_ac(self, flat: abi.FlatCircuit, freqs, vph, want_currents: bool = True) -> dict:
        L = lib()
        d = flat.desc()
        ni, nf = flat.n_inst, len(freqs)
        freqs = np.ascontiguousarray(freqs, dtype=np.float64)
        ph = np.ascontiguousarray(np.broadcast_to(np.asarray(vph, np.complex128).reshape(-1, flat.nV), (ni, flat.nV)))
        out_v = np.zeros((ni, nf, flat.n_out), np.complex128)
        out_i = np.zeros((ni, nf, flat.nR + flat.nC + flat.nL + flat.nV), np.complex128) if want_currents else None
        status = np.full(ni * nf, -1, np.int32)
        skipped = np.zeros(ni * nf, np.int64)
        first = C.c_int64(-1)
        rc = L.spicey_ac_exact_host_run(C.byref(d), self.T, int(self.global_ws), int(self.reverse), nf, _p(freqs, C.c_double),
                                        _p(ph.view(np.float64), C.c_double), _p(out_v.view(np.float64), C.c_double),
                                        _p(out_i.view(np.float64), C.c_double) if want_currents else None, _p(status, C.c_int32),
                                        _p(skipped, C.c_int64), C.byref(first))
        detail = ""
        if rc in (abi.ERR_SINGULAR, abi.ERR_COMPLEX_DIV):
            what = "Singular matrix (complex)" if rc == abi.ERR_SINGULAR else "Complex divide by ~0"
            detail = f"{what} at inst {first.value // max(nf, 1)} frequency index {first.value % max(nf, 1)}"
        return {"status": rc, "detail": detail, "out_v": out_v, "out_i": out_i, "slot_status": status.reshape(ni, nf),
                "skipped": skipped.reshape(ni, nf), "first": first.value}


def plan(flat: abi.FlatCircuit, threads: int = 0, force_global: bool = False, slots: int = 1) -> dict:
    """spicey_ac_exact_plan of the product: {threads, lds, lds_bytes, n, chunk, slot_bytes}, or {rc, error}."""
    L = lib()
    d = flat.desc()
    info = np.zeros(6, np.int64)
    err = C.create_string_buffer(256)
    rc = L.spicey_ac_exact_host_plan(C.byref(d), threads, int(force_global), slots, _p(info, C.c_int64), err, 256)
    if rc != abi.OK:
        return {"rc": rc, "error": err.value.decode()}
    return {"rc": rc, "threads": int(info[0]), "lds": bool(info[1]), "lds_bytes": int(info[2]), "n": int(info[3]), "chunk": int(info[4]),
            "slot_bytes": int(info[5])}


def stamp_lists(flat: abi.FlatCircuit):
    """[((row, column), [(kind, elem, which, sub), ...]), ...] in the order the engine stores them (row-major)."""
    L = lib()
    d = flat.desc()
    nt = C.c_int32(0)
    ne = L.spicey_ac_exact_host_lists(C.byref(d), 0, None, None, 0, None, C.byref(nt))
    assert ne >= 0
    rc = np.zeros((max(ne, 1), 2), np.int32)
    ptr = np.zeros(ne + 1, np.int32)
    terms = np.zeros((max(nt.value, 1), 4), np.int32)
    assert L.spicey_ac_exact_host_lists(C.byref(d), ne, _p(rc, C.c_int32), _p(ptr, C.c_int32), nt.value, _p(terms, C.c_int32), C.byref(nt)) == ne
    kinds = "RCLV"
    return [((int(rc[e, 0]), int(rc[e, 1])), [(kinds[t[0]], int(t[1]), int(t[2]), int(t[3])) for t in terms[ptr[e]:ptr[e + 1]]])
            for e in range(ne)]


def hypot(x, y) -> np.ndarray:
    """The engine's spicey_v8_hypot, elementwise."""
    xy = np.ascontiguousarray(np.stack([np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()], axis=1))
    out = np.empty(len(xy))
    lib().spicey_ac_exact_host_hypot(len(xy), _p(xy, C.c_double), _p(out, C.c_double))
    return out
