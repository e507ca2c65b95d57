"""ctypes binding of libspicey_hip.so — the only compute path of this package.

Loading fails loudly when the shared library is missing (run ``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C spicey_amd/csrc``); creating a handle fails with
SPICEY_ERR_NO_DEVICE when there is no GPU.  Nothing here falls back to a CPU solver.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPICEY_HIP_LIB") or os.path.join(_HERE, "libspicey_hip.so")  # same override as ts/spiceyHip.ts
_LIB = None

_i32, _i64, _f64, _vp, _str = C.c_int32, C.c_int64, C.c_double, C.c_void_p, C.c_char_p
_f64p, _i32p, _i64p, _u64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
_descp, _optp, _infop, _outp = C.POINTER(abi.SpiceyDesc), C.POINTER(abi.SpiceyOptions), C.POINTER(abi.SpiceyInfo), C.POINTER(C.c_void_p)
# name -> (restype, argtypes) of every function include/spicey_hip.h declares: load() binds them, EXPORTS lists them
SIGNATURES = {
    "spicey_create": (_i32, [_descp, _optp, _outp]),
    "spicey_run": (_i32, [_vp, _i64, _f64, _f64p, _f64p, _f64p, _i32p]),
    "spicey_run_device": (_i32, [_vp, _i64, _f64, _vp, _vp, _vp, _vp, _vp]),
    "spicey_run_src": (_i32, [_vp, _i64, _f64, _f64p, _i32, _f64p, _f64p, _i32p]),
    "spicey_run_device_src": (_i32, [_vp, _i64, _f64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "spicey_last_inst_status": (_i32, [_vp, _i32p]),
    "spicey_sync": (_i32, [_vp]),
    "spicey_get_state": (_i32, [_vp, _f64p, _f64p, _f64p, _i32p]),
    "spicey_set_state": (_i32, [_vp, _f64p, _f64p, _f64p, _i32p]),
    "spicey_reset_state": (_i32, [_vp, _vp]),
    "spicey_last_solve_count": (_i64, [_vp]),
    "spicey_group_retries": (_i32, [_vp]),
    "spicey_group_stale_polls": (_i64, [_vp]),
    "spicey_last_skip_risk": (_i64, [_vp, _i64p]),
    "spicey_get_lin_err": (_i32, [_vp, _f64p]),
    "spicey_last_kernel_ms": (_f64, [_vp]),
    "spicey_get_info": (_i32, [_vp, _infop]),
    "spicey_top_regs_form": (_i32, [_vp, _i64]),
    "spicey_u0_resident_form": (_i32, [_vp, _i64]),
    "spicey_top_fold_form": (_i32, [_vp, _i64]),
    "spicey_stamp_fuse_form": (_i32, [_vp, _i64]),
    "spicey_fixed_schedule_form": (_i32, [_vp, _i64]),
    "spicey_last_error": (_str, [_vp]),
    "spicey_destroy": (None, [_vp]),
    "spicey_version": (_str, []),
    "spicey_debug_phase_cycles": (_i32, [_vp, _u64p, _i32]),
    "spicey_debug_phase_cycles_wg": (_i32, [_vp, _i32, _u64p, _i32]),
    "spicey_debug_front_ticks": (_i32, [_vp, _i32, _u64p, _i32p, _i32]),
    "spicey_create_multi": (_i32, [_descp, _optp, _i32p, _i32, _outp]),
    "spicey_run_multi": (_i32, [_vp, _i64, _f64, _f64p, _f64p, _f64p, _i32p]),
    "spicey_run_multi_src": (_i32, [_vp, _i64, _f64, _f64p, _i32, _f64p, _f64p, _i32p]),
    "spicey_get_state_multi": (_i32, [_vp, _f64p, _f64p, _f64p, _i32p]),
    "spicey_multi_get_shard": (_i32, [_vp, _i32, _infop, _i32p, _i32p, _i32p]),
    "spicey_multi_last_solve_count": (_i64, [_vp]),
    "spicey_multi_group_retries": (_i32, [_vp]),
    "spicey_multi_group_stale_polls": (_i64, [_vp]),
    "spicey_multi_last_kernel_ms": (_f64, [_vp]),
    "spicey_multi_last_error": (_str, [_vp]),
    "spicey_destroy_multi": (None, [_vp]),
    "spicey_ac_create": (_i32, [_descp, _optp, _outp]),
    "spicey_ac_run": (_i32, [_vp, _i64, _f64p, _f64p, _f64p, _f64p]),
    "spicey_ac_get_info": (_i32, [_vp, _infop]),
    "spicey_ac_last_kernel_ms": (_f64, [_vp]),
    "spicey_ac_last_error": (_str, [_vp]),
    "spicey_ac_destroy": (None, [_vp]),
    "spicey_format_tran": (_i64, [_i64, _i32, _f64p, _f64p, _i64, _i32p, _str, _str, _i64]),
    "spicey_to_precision6": (_i32, [_f64, _str]),
    "spicey_measure_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "spicey_measure_device": (_i32, [_i32, _i32, _i64, _f64, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i64, _vp]),
    "spicey_run_measure": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _i32, _f64p, _i32p]),
    "spicey_last_measure_ms": (_f64, [_vp]),
    "spicey_fourier_workspace_bytes": (_i64, [_i32, _i64, _vp, _i32]),
    "spicey_fourier_device": (_i32, [_i32, _i32, _i64, _f64, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i64, _vp]),
    "spicey_run_measure_fourier": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _i32, _f64p, _vp, _i32, _f64p, _i32, _i32p]),
    "spicey_last_fourier_ms": (_f64, [_vp]),
    "spicey_timing_workspace_bytes": (_i64, [_i32, _i64, _vp, _i32]),
    "spicey_timing_device": (_i32, [_i32, _i32, _i64, _f64, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i64, _vp]),
    "spicey_run_measure_timing": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _i32, _f64p, _vp, _i32, _f64p, _i32, _vp, _i32, _f64p, _i32p]),
    "spicey_last_timing_ms": (_f64, [_vp]),
    "spicey_spectrum_workspace_bytes": (_i64, [_i32, _i64, _vp, _i32]),
    "spicey_spectrum_device": (_i32, [_i32, _i32, _i64, _f64, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i64, _vp]),
    "spicey_run_measure_spectrum": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _i32, _f64p, _vp, _i32, _f64p, _i32, _vp, _i32, _f64p, _vp, _i32, _f64p, _i32,
                                           _i32p]),
    "spicey_last_spectrum_ms": (_f64, [_vp]),
    "spicey_power_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "spicey_power_device": (_i32, [_i32, _i32, _i64, _f64, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i64, _vp]),
    "spicey_run_measure_power": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _i32, _f64p, _vp, _i32, _f64p, _i32, _vp, _i32, _f64p, _vp, _i32, _f64p, _i32,
                                        _vp, _i32, _f64p, _i32p]),
    "spicey_last_power_ms": (_f64, [_vp]),
    "spicey_values_workspace_bytes": (_i64, [_i32, _i64, _vp, _i32, _i64]),
    "spicey_values_device": (_i32, [_i32, _i32, _i64, _f64, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i64, _vp, _i32, _vp, _i32, _vp, _i64, _vp]),
    "spicey_run_reduced": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _i32p]),
    "spicey_last_values_ms": (_f64, [_vp]),
    "spicey_ac_last_inst_status": (_i32, [_vp, _i32p, _i64p]),
    "spicey_ac_measure_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "spicey_ac_measure_device": (_i32, [_i32, _i32, _i64, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i64, _vp]),
    "spicey_ac_run_measure": (_i32, [_vp, _i64, _f64p, _f64p, _vp, _i32, _f64p]),
    "spicey_ac_last_measure_ms": (_f64, [_vp]),
    "spicey_ac_run_inject": (_i32, [_vp, _i64, _f64p, _f64p, _vp, _f64p, _f64p]),
    "spicey_ac_noise_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "spicey_ac_noise_device": (_i32, [_i32, _i32, _i64, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_ac_run_noise": (_i32, [_vp, _i64, _f64p, _f64p, _vp, _vp, _f64p, _f64p, _f64p, _f64p]),
    "spicey_ac_last_noise_ms": (_f64, [_vp]),
    "spicey_ac_sens_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "spicey_ac_sens_device": (_i32, [_i32, _i32, _i64, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _f64p, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_ac_run_sens": (_i32, [_vp, _i64, _f64p, _f64p, _vp, _vp, _f64p, _f64p, _f64p, _f64p]),
    "spicey_ac_last_sens_ms": (_f64, [_vp]),
    "spicey_ac_mc_workspace_bytes": (_i64, [_i32, _i64, _i32, _i32, _i32]),
    "spicey_ac_mc_draw_device": (_i32, [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f64p, _f64p, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_ac_mc_reduce_device": (_i32, [_i32, _i32, _i64, _vp, _i32, _vp, _f64p, _f64p, _i64p, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_ac_run_mc": (_i32, [_vp, _i64, _f64p, _f64p, _vp, _f64p, _f64p, _f64p, _f64p, _f64p, _i32, _f64p, _i64p, _f64p]),
    "spicey_ac_last_mc_ms": (_f64, [_vp]),
    "spicey_ac_last_mc_draw_ms": (_f64, [_vp]),
    "spicey_tran_mc_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "spicey_tran_mc_draw_device": (_i32, [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _f64p, _f64p, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_tran_mc_reduce_device": (_i32, [_i32, _i32, _vp, _vp, _i32, _vp, _f64p, _f64p, _f64p, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_run_mc": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _vp, _f64p, _f64p, _vp, _i32, _f64p, _f64p, _f64p, _i32, _f64p, _i64p, _f64p, _i32p]),
    "spicey_last_tran_mc_ms": (_f64, [_vp]),
    "spicey_last_tran_mc_draw_ms": (_f64, [_vp]),
    "spicey_tran_sens_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "spicey_tran_sens_design_device": (_i32, [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_tran_sens_reduce_device": (_i32, [_i32, _i32, _vp, _vp, _i32, _vp, _f64p, _f64p, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_run_sens": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _vp, _vp, _f64p, _f64p, _vp, _i32, _f64p, _vp, _f64p, _f64p, _i32p]),
    "spicey_run_levels": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _vp, _vp, _f64p, _vp, _i32, _f64p, _i32p]),
    "spicey_last_tran_sens_ms": (_f64, [_vp]),
    "spicey_last_tran_sens_design_ms": (_f64, [_vp]),
    "spicey_pss_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "spicey_pss_design_device": (_i32, [_i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_pss_update_device": (_i32, [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_run_pss": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _f64p, _i32p, _f64p, _i32p, _i32p]),
    "spicey_last_pss_ms": (_f64, [_vp]),
    "spicey_last_pss_tran_ms": (_f64, [_vp]),
    "spicey_fit_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "spicey_fit_design_device": (_i32, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_fit_update_device": (_i32, [_i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "spicey_run_fit": (_i32, [_vp, _i64, _f64, _f64p, _i32, _vp, _vp, _vp, _f64p, _f64p, _f64p, _f64p, _vp, _vp, _i32, _f64p, _f64p, _f64p, _i32p, _i32p,
                              _f64p, _i32p]),
    "spicey_last_fit_ms": (_f64, [_vp]),
    "spicey_last_fit_tran_ms": (_f64, [_vp]),
}
EXPORTS = list(SIGNATURES)


class SpiceyNativeError(RuntimeError):
    pass


def _fail(what: str, rc: int, msg) -> None:
    """Raises SpiceyNativeError for the library's status `rc` (kept as `.status`) and its message (bytes or str)."""
    err = SpiceyNativeError(f"{what} failed ({rc}): {msg.decode() if isinstance(msg, bytes) else msg or ''}")
    err.status = rc
    raise err


# Group mode health of this process: launches repeated after a bounded-wait abort and waits that only the read-modify-write
# poll saw satisfied, summed over every handle closed so far (include/spicey_hip.h: spicey_group_retries,
# spicey_group_stale_polls).  Both stay 0 in a healthy process; the GPU tests assert that around every test.
GROUP_TOTALS = {"retries": 0, "stale_polls": 0}


def load():
    """The library, opened on first use.  In a process that also uses torch, whose wheel brings a HIP runtime of its own:
    open the library (any function of this module) either after torch has touched the device or by a call that itself
    initialises HIP (a Handle); opening it first, letting torch initialise, and only then making the first HIP call through
    the library has been seen to answer "no HIP device"."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise SpiceyNativeError(f"{LIB_PATH} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                                "spicey_amd has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = L
    return L


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _src_layout(src: np.ndarray, f: abi.FlatCircuit, steps: int) -> bool:
    """True for one table per instance [n_inst][steps+1][nV], False for one shared [steps+1][nV]; anything else raises."""
    if src.shape == (steps + 1, f.nV):
        return False
    if src.shape == (f.n_inst, steps + 1, f.nV):
        return True
    raise ValueError(f"src_table must be [steps+1][nV] = {(steps + 1, f.nV)} or [n_inst][steps+1][nV] = {(f.n_inst, steps + 1, f.nV)}, "
                     f"got {src.shape}")


def _reqs(reqs, dtype=abi.MEAS_REQ_DTYPE) -> np.ndarray:
    """A request list as one contiguous array of records of `dtype` (abi.MEAS_REQ_DTYPE, FOUR_, TIMING_, AC_MEAS_REQ_DTYPE)."""
    return np.ascontiguousarray(reqs, dtype=dtype).reshape(-1)


def _reqs_ptr(r: np.ndarray):
    return r.ctypes.data if len(r) else None


def _state_arrays(f: abi.FlatCircuit):
    """A zeroed state dict of `f`'s instances and its arrays as the arguments of spicey_get_state(_multi)."""
    st = {"C_vprev": np.zeros((f.n_inst, f.nC)), "L_iprev": np.zeros((f.n_inst, f.nL)), "D_vdprev": np.zeros((f.n_inst, f.nD)),
          "S_ison": np.zeros((f.n_inst, f.nS), np.int32)}
    return st, (_p(st["C_vprev"], C.c_double), _p(st["L_iprev"], C.c_double), _p(st["D_vdprev"], C.c_double), _p(st["S_ison"], C.c_int32))


def measure_workspace_bytes(n_inst: int, n_points: int, n_req: int) -> int:
    return load().spicey_measure_workspace_bytes(n_inst, n_points, n_req)


def ac_measure_workspace_bytes(n_inst: int, n_freq: int, n_req: int) -> int:
    return load().spicey_ac_measure_workspace_bytes(n_inst, n_freq, n_req)


def _measure_device(fn: str, shape: tuple, d_v: int, n_v: int, d_i: int, n_i: int, r: np.ndarray, d_meas: int, d_work: int, work_bytes: int,
                    device: int, stream: int) -> None:
    L = load()
    rc = getattr(L, fn)(device, *shape, d_v or None, n_v, d_i or None, n_i, _reqs_ptr(r), len(r), d_meas or None, d_work or None, work_bytes,
                        stream or None)
    if rc != abi.OK:
        _fail(fn, rc, L.spicey_last_error(None))


def measure_device(n_inst: int, n_points: int, dt: float, d_v: int, n_v: int, d_i: int, n_i: int, reqs, d_meas: int, d_work: int,
                   work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_measure_device: the reduction alone on raw device pointers (e.g. torch tensors' data_ptr()): d_v
    [n_inst][n_points][n_v], d_i [n_inst][n_points][n_i] or 0, d_meas [n_inst][n_req][8], d_work of `work_bytes` >=
    measure_workspace_bytes(...).  Enqueued on `stream`, no synchronisation.  A refusal raises SpiceyNativeError whose
    `status` is the library's code (abi.ERR_BAD_DESC for a bad request list)."""
    _measure_device("spicey_measure_device", (n_inst, n_points, dt), d_v, n_v, d_i, n_i, _reqs(reqs), d_meas, d_work, work_bytes, device, stream)


def ac_measure_device(n_inst: int, n_freq: int, d_v: int, n_v: int, d_i: int, n_i: int, reqs, d_meas: int, d_work: int, work_bytes: int,
                      device: int = 0, stream: int = 0) -> None:
    """The same for an AC sweep's buffers (spicey_ac_measure_device): d_v [n_inst][n_freq][n_v] complex128, d_i likewise or
    0, d_work of `work_bytes` >= ac_measure_workspace_bytes(...)."""
    _measure_device("spicey_ac_measure_device", (n_inst, n_freq), d_v, n_v, d_i, n_i, _reqs(reqs, abi.AC_MEAS_REQ_DTYPE), d_meas, d_work, work_bytes, device, stream)


def ac_noise_workspace_bytes(n_inst: int, n_freq: int, nR: int) -> int:
    return load().spicey_ac_noise_workspace_bytes(n_inst, n_freq, nR)


def ac_noise_device(n_inst: int, n_freq: int, d_v: int, n_v: int, d_i: int, n_i: int, d_R: int, nR: int, d_freqs: int, req: abi.SpiceyAcNoiseReq,
                    d_spec: int, d_contrib: int, d_total: int, d_work: int, work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_ac_noise_device: the noise pass alone on raw device pointers: d_v [n_inst][n_freq][n_v] and d_i
    [n_inst][n_freq][n_i] complex128 of an injected sweep, d_R [n_inst][nR] ohms, d_freqs [n_freq], d_spec [n_inst][n_freq][4],
    d_contrib [n_inst][nR], d_total [n_inst][2], d_work of `work_bytes` >= ac_noise_workspace_bytes(...).  Enqueued on `stream`,
    no synchronisation.  A refusal raises SpiceyNativeError whose `status` is abi.ERR_BAD_DESC."""
    L = load()
    rc = L.spicey_ac_noise_device(device, n_inst, n_freq, d_v or None, n_v, d_i or None, n_i, d_R or None, nR, d_freqs or None,
                                  C.byref(req) if req is not None else None, d_spec or None, d_contrib or None, d_total or None, d_work or None,
                                  work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_ac_noise_device", rc, L.spicey_last_error(None))


def ac_sens_workspace_bytes(n_inst: int, n_freq: int, nE: int) -> int:
    return load().spicey_ac_sens_workspace_bytes(n_inst, n_freq, nE)


def ac_sens_device(n_inst: int, n_freq: int, d_v_dir: int, n_v: int, d_i_dir: int, d_i_adj: int, n_i: int, d_R: int, d_C: int, d_L: int, tol, d_freqs: int,
                   req: abi.SpiceyAcSensReq, d_spec: int, d_peak: int, d_full: int, d_work: int, work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_ac_sens_device: the sensitivity pass alone on raw device pointers: d_v_dir [n_inst][n_freq][n_v] and d_i_dir
    [n_inst][n_freq][n_i] complex128 of the plain sweep, d_i_adj likewise of the injected one, d_R / d_C / d_L [n_inst][n<kind>]
    (0 where the count is 0), d_freqs [n_freq], d_spec [n_inst][n_freq][6], d_peak [n_inst][nE][4], d_full [n_inst][n_freq][nE][2]
    or 0, d_work of `work_bytes` >= ac_sens_workspace_bytes(...).  tol [nE] is a HOST array (None stands for a null pointer).
    Enqueued on `stream`, no synchronisation.  A refusal raises SpiceyNativeError whose `status` is abi.ERR_BAD_DESC."""
    L = load()
    t = None if tol is None else np.ascontiguousarray(tol, dtype=np.float64)
    rc = L.spicey_ac_sens_device(device, n_inst, n_freq, d_v_dir or None, n_v, d_i_dir or None, d_i_adj or None, n_i, d_R or None, d_C or None, d_L or None,
                                 _p(t, C.c_double), d_freqs or None, C.byref(req) if req is not None else None, d_spec or None, d_peak or None,
                                 d_full or None, d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_ac_sens_device", rc, L.spicey_last_error(None))


def ac_mc_workspace_bytes(n_inst: int, n_freq: int, nE: int, log2K: int, n_rank: int) -> int:
    return load().spicey_ac_mc_workspace_bytes(n_inst, n_freq, nE, log2K, n_rank)


def _host(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def ac_mc_draw_device(n_inst: int, nR: int, nC: int, nL: int, d_R: int, d_C: int, d_L: int, tol, icdf, req: abi.SpiceyAcMcReq, d_Rinv_out: int, d_C_out: int,
                      d_L_out: int, d_work: int, work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_ac_mc_draw_device: the Monte Carlo draw alone on raw device pointers: d_R (ohms), d_C, d_L nominal [n_inst][n<kind>],
    the three drawn arrays of the same shapes (the first as 1 / ohms), 0 where the count is 0, d_work of `work_bytes` >=
    ac_mc_workspace_bytes(...).  tol [nE] and icdf [2^log2K + 1] are HOST arrays (None stands for a null pointer).  Enqueued on
    `stream`, no synchronisation.  A refusal raises SpiceyNativeError whose `status` is abi.ERR_BAD_DESC."""
    L = load()
    t, tab = _host(tol, np.float64), _host(icdf, np.float64)
    rc = L.spicey_ac_mc_draw_device(device, n_inst, nR, nC, nL, d_R or None, d_C or None, d_L or None, _p(t, C.c_double), _p(tab, C.c_double),
                                    C.byref(req) if req is not None else None, d_Rinv_out or None, d_C_out or None, d_L_out or None, d_work or None, work_bytes,
                                    stream or None)
    if rc != abi.OK:
        _fail("spicey_ac_mc_draw_device", rc, L.spicey_last_error(None))


def ac_mc_reduce_device(n_inst: int, n_freq: int, d_v: int, n_v: int, valid, lo, hi, ranks, req: abi.SpiceyAcMcReq, d_sample: int, d_freq: int, d_work: int,
                        work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_ac_mc_reduce_device: the reduction across instances alone on raw device pointers: d_v [n_inst][n_freq][n_v]
    complex128, d_sample [n_inst][2] int64, d_freq [n_freq][4 + n_rank], d_work.  valid [n_inst] (bytes, None: all), lo / hi
    [n_freq] (None: no limit) and ranks [n_rank] are HOST arrays.  Enqueued on `stream`, no synchronisation."""
    L = load()
    va, lo_, hi_, rk = _host(valid, np.uint8), _host(lo, np.float64), _host(hi, np.float64), _host(ranks, np.int64)
    rc = L.spicey_ac_mc_reduce_device(device, n_inst, n_freq, d_v or None, n_v, va.ctypes.data if va is not None else None, _p(lo_, C.c_double),
                                      _p(hi_, C.c_double), _p(rk, C.c_int64) if rk is not None and len(rk) else None, len(rk) if rk is not None else 0,
                                      C.byref(req) if req is not None else None, d_sample or None, d_freq or None, d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_ac_mc_reduce_device", rc, L.spicey_last_error(None))


def tran_mc_workspace_bytes(n_inst: int, n_scalar: int, nE: int, log2K: int, n_prob: int) -> int:
    return load().spicey_tran_mc_workspace_bytes(n_inst, n_scalar, nE, log2K, n_prob)


def tran_mc_draw_device(n_inst: int, nR: int, nC: int, nL: int, d_R: int, d_C: int, d_L: int, tol, icdf, req: abi.SpiceyTranMcReq, d_R_out: int, d_C_out: int,
                        d_L_out: int, d_work: int, work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_tran_mc_draw_device: ac_mc_draw_device's draw with the resistors left in ohms, as a transient run reads them."""
    L = load()
    t, tab = _host(tol, np.float64), _host(icdf, np.float64)
    rc = L.spicey_tran_mc_draw_device(device, n_inst, nR, nC, nL, d_R or None, d_C or None, d_L or None, _p(t, C.c_double), _p(tab, C.c_double),
                                      C.byref(req) if req is not None else None, d_R_out or None, d_C_out or None, d_L_out or None, d_work or None, work_bytes,
                                      stream or None)
    if rc != abi.OK:
        _fail("spicey_tran_mc_draw_device", rc, L.spicey_last_error(None))


def _mc_rows(rows):
    """(abi.SpiceyMcRows * 3) of rows = [(device pointer, n_rows, stride)] for measure, timing, power."""
    arr = (abi.SpiceyMcRows * 3)()
    for k, (ptr, n_rows, stride) in enumerate(rows):
        arr[k].d_rows, arr[k].n_rows, arr[k].stride = ptr or None, int(n_rows), int(stride)
    return arr


def _scalars(scalars) -> np.ndarray:
    return np.ascontiguousarray(scalars, dtype=abi.MC_SCALAR_DTYPE).reshape(-1)


def tran_mc_reduce_device(n_inst: int, rows, scalars, valid, lo, hi, probs, d_x: int, d_stat: int, d_sample: int, d_work: int, work_bytes: int,
                          device: int = 0, stream: int = 0, n_scalar: Optional[int] = None) -> None:
    """spicey_tran_mc_reduce_device: the scalars and the reduction across instances alone on raw device pointers.  rows: three
    (device pointer, n_rows, stride) for the measure, timing and power rows (None stands for a null list); scalars: records of
    abi.MC_SCALAR_DTYPE; valid [n_inst] (bytes, None: all), lo / hi [n_scalar] (None: no limit) and probs are HOST arrays; d_x
    [n_inst][n_scalar], d_stat [n_scalar][8 + 2 n_prob], d_sample [n_inst][2] int64.  Enqueued on `stream`, no synchronisation."""
    L = load()
    sc = None if scalars is None else _scalars(scalars)
    va, lo_, hi_, pr = _host(valid, np.uint8), _host(lo, np.float64), _host(hi, np.float64), _host(probs, np.float64)
    mr = None if rows is None else _mc_rows(rows)
    rc = L.spicey_tran_mc_reduce_device(device, n_inst, None if mr is None else C.addressof(mr), sc.ctypes.data if sc is not None and len(sc) else None,
                                        (len(sc) if sc is not None else 0) if n_scalar is None else n_scalar, va.ctypes.data if va is not None else None,
                                        _p(lo_, C.c_double), _p(hi_, C.c_double), _p(pr, C.c_double) if pr is not None and len(pr) else None,
                                        len(pr) if pr is not None else 0, d_x or None, d_stat or None, d_sample or None, d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_tran_mc_reduce_device", rc, L.spicey_last_error(None))


def tran_sens_workspace_bytes(n_inst: int, n_scalar: int, nE: int, nA: int) -> int:
    return load().spicey_tran_sens_workspace_bytes(n_inst, n_scalar, nE, nA)


def _data(a):
    return a.ctypes.data if a is not None and a.size else None


def tran_sens_design_device(n_inst: int, nR: int, nC: int, nL: int, d_R: int, d_C: int, d_L: int, req: abi.SpiceyTranSensReq, act, step, lvl, tol, d_R_out: int,
                            d_C_out: int, d_L_out: int, d_work: int, work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_tran_sens_design_device: the deterministic design — ONE_AT_A_TIME from act [nA] (int32) and step [nA], or LEVELS from
    lvl [n_inst][nE] (int8) and tol [nE], HOST arrays — written into raw device value arrays, the resistors in ohms."""
    L = load()
    ac, st, lv, tl = _host(act, np.int32), _host(step, np.float64), _host(lvl, np.int8), _host(tol, np.float64)
    rc = L.spicey_tran_sens_design_device(device, n_inst, nR, nC, nL, d_R or None, d_C or None, d_L or None, C.addressof(req) if req is not None else None, _data(ac),
                                          _data(st), _data(lv), _data(tl), d_R_out or None, d_C_out or None, d_L_out or None, d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_tran_sens_design_device", rc, L.spicey_last_error(None))


def tran_sens_reduce_device(n_inst: int, rows, scalars, valid, step, tol_act, d_x: int, d_sens: int, d_sign: int, d_bound: int, d_work: int, work_bytes: int,
                            device: int = 0, stream: int = 0, nA: Optional[int] = None) -> None:
    """spicey_tran_sens_reduce_device: the scalars and the reduction of a one-at-a-time design alone on raw device pointers.  rows,
    scalars and valid as for tran_mc_reduce_device; step [nA] and tol_act [nA] are HOST arrays; d_x [n_inst][n_scalar], d_sens
    [n_scalar][nA][2], d_sign [n_scalar][nA] int8, d_bound [n_scalar][8].  Enqueued on `stream`, no synchronisation."""
    L = load()
    sc = None if scalars is None else _scalars(scalars)
    va, st, tl = _host(valid, np.uint8), _host(step, np.float64), _host(tol_act, np.float64)
    mr = None if rows is None else _mc_rows(rows)
    rc = L.spicey_tran_sens_reduce_device(device, n_inst, None if mr is None else C.addressof(mr), sc.ctypes.data if sc is not None and len(sc) else None,
                                          len(sc) if sc is not None else 0, va.ctypes.data if va is not None else None, _p(st, C.c_double), _p(tl, C.c_double),
                                          (len(st) if st is not None else 0) if nA is None else nA, d_x or None, d_sens or None, d_sign or None, d_bound or None,
                                          d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_tran_sens_reduce_device", rc, L.spicey_last_error(None))


def pss_workspace_bytes(n_ckt: int, nX: int, method: int = abi.PSS_NEWTON) -> int:
    return load().spicey_pss_workspace_bytes(n_ckt, nX, method)


def pss_design_device(kinds, nS: int, req: abi.SpiceyPssReq, d_base: int, d_base_on: int, d_h: int, d_Cv: int, d_Li: int, d_Dv: int, d_Son: int, d_work: int,
                      work_bytes: int, perturb: bool = True, device: int = 0, stream: int = 0) -> None:
    """spicey_pss_design_device: the design over the state alone on raw device pointers: d_base [n_ckt][nX], d_base_on [n_ckt][nS],
    d_h [n_ckt][nX] and the state arrays [n_ckt W][n<kind>] (0 where the count is 0); kinds = (nC, nL, nD).  Enqueued on `stream`,
    no synchronisation.  A refusal raises SpiceyNativeError whose `status` is abi.ERR_BAD_DESC."""
    L = load()
    rc = L.spicey_pss_design_device(device, *kinds, nS, C.addressof(req) if req is not None else None, int(perturb), d_base or None, d_base_on or None, d_h or None,
                                    d_Cv or None, d_Li or None, d_Dv or None, d_Son or None, d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_pss_design_device", rc, L.spicey_last_error(None))


def pss_update_device(kinds, nS: int, req: abi.SpiceyPssReq, inst_status, d_base: int, d_base_on: int, d_h: int, d_Cv: int, d_Li: int, d_Dv: int, d_Son: int,
                      d_delta: int, d_rows: int, d_done: int, d_work: int, work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_pss_update_device: the Newton update alone on raw device pointers; the state arrays hold the END states, inst_status
    [n_ckt W] is a HOST array (None: all 0); d_base, d_base_on, d_delta [n_ckt][nX] (or 0), d_rows [n_ckt][8] and d_done [n_ckt]
    are written.  Enqueued on `stream`, no synchronisation."""
    L = load()
    ist = _host(inst_status, np.int32)
    rc = L.spicey_pss_update_device(device, *kinds, nS, C.addressof(req) if req is not None else None, _data(ist), d_base or None, d_base_on or None, d_h or None,
                                    d_Cv or None, d_Li or None, d_Dv or None, d_Son or None, d_delta or None, d_rows or None, d_done or None, d_work or None, work_bytes,
                                    stream or None)
    if rc != abi.OK:
        _fail("spicey_pss_update_device", rc, L.spicey_last_error(None))


def fit_workspace_bytes(n_ckt: int, nA: int, n_scalar: int) -> int:
    return load().spicey_fit_workspace_bytes(n_ckt, nA, n_scalar)


def _goals(goals) -> Optional[np.ndarray]:
    return None if goals is None else np.ascontiguousarray(goals, dtype=abi.FIT_GOAL_DTYPE).reshape(-1)


def fit_design_device(nR: int, nC: int, nL: int, d_R: int, d_C: int, d_L: int, req: abi.SpiceyFitReq, act, step, d_g: int, d_R_out: int, d_C_out: int, d_L_out: int,
                      d_work: int, work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_fit_design_device: the design over the gains d_g [n_ckt][nA] alone on raw device pointers; act [nA] (int32) and step
    [nA] are HOST arrays, the value arrays [n_ckt (1 + 2 nA)][n<kind>] (0 where the count is 0), the resistors in ohms.  Enqueued
    on `stream`, no synchronisation.  A refusal raises SpiceyNativeError whose `status` is abi.ERR_BAD_DESC."""
    L = load()
    ac, st = _host(act, np.int32), _host(step, np.float64)
    rc = L.spicey_fit_design_device(device, nR, nC, nL, d_R or None, d_C or None, d_L or None, C.addressof(req) if req is not None else None, _data(ac), _data(st),
                                    d_g or None, d_R_out or None, d_C_out or None, d_L_out or None, d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_fit_design_device", rc, L.spicey_last_error(None))


def fit_update_device(req: abi.SpiceyFitReq, n_scalar: int, first: bool, step, g_lo, g_hi, goals, valid, d_x: int, d_g: int, d_rows: int, d_done: int, d_work: int,
                      work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_fit_update_device: the damped least-squares update alone on raw device pointers: d_x [n_inst][n_scalar], d_g
    [n_ckt][nA], d_rows [n_ckt][8], d_done [n_ckt]; step [nA], g_lo / g_hi [n_ckt][nA], goals [n_ckt][n_scalar] (records of
    abi.FIT_GOAL_DTYPE) and valid [n_inst] (bytes, None: all) are HOST arrays.  d_work carries the circuits' state from one update to
    the next.  Enqueued on `stream`, no synchronisation."""
    L = load()
    st, lo, hi, go, va = _host(step, np.float64), _host(g_lo, np.float64), _host(g_hi, np.float64), _goals(goals), _host(valid, np.uint8)
    rc = L.spicey_fit_update_device(device, C.addressof(req) if req is not None else None, n_scalar, int(bool(first)), _data(st), _data(lo), _data(hi), _data(go),
                                    _data(va), d_x or None, d_g or None, d_rows or None, d_done or None, d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_fit_update_device", rc, L.spicey_last_error(None))


def fourier_row_doubles(reqs) -> int:
    """Doubles of a result row that holds every request of the list: 1 + 2 max n_harm."""
    r = _reqs(reqs, abi.FOUR_REQ_DTYPE)
    return 1 + 2 * int(r["n_harm"].max()) if len(r) else 1


def fourier_workspace_bytes(n_inst: int, n_points: int, reqs) -> int:
    """spicey_fourier_workspace_bytes: device workspace of fourier_device for this request list; -1 for a refused one."""
    r = _reqs(reqs, abi.FOUR_REQ_DTYPE)
    return load().spicey_fourier_workspace_bytes(n_inst, n_points, _reqs_ptr(r), len(r))


def fourier_device(n_inst: int, n_points: int, dt: float, d_v: int, n_v: int, d_i: int, n_i: int, reqs, d_out: int, out_stride: int, d_work: int,
                   work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_fourier_device: the harmonics pass alone on raw device pointers (e.g. torch tensors' data_ptr()): d_v
    [n_inst][n_points][n_v], d_i [n_inst][n_points][n_i] or 0, d_out [n_inst][n_req][out_stride], d_work of `work_bytes` >=
    fourier_workspace_bytes(...).  reqs: records of abi.FOUR_REQ_DTYPE.  Enqueued on `stream`, no synchronisation.  A
    refusal raises SpiceyNativeError whose `status` is the library's code (abi.ERR_BAD_DESC for a bad request list)."""
    L = load()
    r = _reqs(reqs, abi.FOUR_REQ_DTYPE)
    rc = L.spicey_fourier_device(device, n_inst, n_points, dt, d_v or None, n_v, d_i or None, n_i, _reqs_ptr(r), len(r), d_out or None, out_stride,
                                 d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_fourier_device", rc, L.spicey_last_error(None))


def timing_workspace_bytes(n_inst: int, n_points: int, reqs) -> int:
    """spicey_timing_workspace_bytes: device workspace of timing_device for this request list; -1 for a refused one."""
    r = _reqs(reqs, abi.TIMING_REQ_DTYPE)
    return load().spicey_timing_workspace_bytes(n_inst, n_points, _reqs_ptr(r), len(r))


def timing_device(n_inst: int, n_points: int, dt: float, d_v: int, n_v: int, d_i: int, n_i: int, reqs, d_out: int, d_work: int, work_bytes: int,
                  device: int = 0, stream: int = 0) -> None:
    """spicey_timing_device: the edge-timing pass alone on raw device pointers (e.g. torch tensors' data_ptr()): d_v
    [n_inst][n_points][n_v], d_i [n_inst][n_points][n_i] or 0, d_out [n_inst][n_req][8], d_work of `work_bytes` >=
    timing_workspace_bytes(...).  reqs: records of abi.TIMING_REQ_DTYPE.  Enqueued on `stream`, no synchronisation.  A
    refusal raises SpiceyNativeError whose `status` is the library's code (abi.ERR_BAD_DESC for a bad request list)."""
    _measure_device("spicey_timing_device", (n_inst, n_points, dt), d_v, n_v, d_i, n_i, _reqs(reqs, abi.TIMING_REQ_DTYPE), d_out, d_work, work_bytes, device, stream)


def spectrum_workspace_bytes(n_inst: int, n_points: int, reqs) -> int:
    """spicey_spectrum_workspace_bytes: device workspace of spectrum_device for this request list; -1 for a refused one."""
    r = _reqs(reqs, abi.SPEC_REQ_DTYPE)
    return load().spicey_spectrum_workspace_bytes(n_inst, n_points, _reqs_ptr(r), len(r))


def spectrum_device(n_inst: int, n_points: int, dt: float, d_v: int, n_v: int, d_i: int, n_i: int, reqs, d_out: int, out_stride: int, d_work: int,
                    work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_spectrum_device: the spectrum pass alone on raw device pointers (e.g. torch tensors' data_ptr()): d_v
    [n_inst][n_points][n_v], d_i [n_inst][n_points][n_i] or 0, d_out [n_inst][n_req][out_stride], d_work of `work_bytes` >=
    spectrum_workspace_bytes(...).  reqs: records of abi.SPEC_REQ_DTYPE.  Enqueued on `stream`, no synchronisation.  A
    refusal raises SpiceyNativeError whose `status` is the library's code (abi.ERR_BAD_DESC for a bad request list)."""
    L = load()
    r = _reqs(reqs, abi.SPEC_REQ_DTYPE)
    rc = L.spicey_spectrum_device(device, n_inst, n_points, dt, d_v or None, n_v, d_i or None, n_i, _reqs_ptr(r), len(r), d_out or None, out_stride,
                                  d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_spectrum_device", rc, L.spicey_last_error(None))


def power_workspace_bytes(n_inst: int, n_points: int, n_req: int) -> int:
    """spicey_power_workspace_bytes: device workspace of power_device; -1 for counts <= 0."""
    return load().spicey_power_workspace_bytes(n_inst, n_points, n_req)


def power_device(n_inst: int, n_points: int, dt: float, d_v: int, n_v: int, d_i: int, n_i: int, reqs, d_out: int, d_work: int, work_bytes: int,
                 device: int = 0, stream: int = 0) -> None:
    """spicey_power_device: the product pass alone on raw device pointers (e.g. torch tensors' data_ptr()): d_v
    [n_inst][n_points][n_v], d_i [n_inst][n_points][n_i] or 0, d_out [n_inst][n_req][abi.POWER_ROW], d_work of `work_bytes` >=
    power_workspace_bytes(...).  reqs: records of abi.POWER_REQ_DTYPE.  Enqueued on `stream`, no synchronisation.  A refusal
    raises SpiceyNativeError whose `status` is the library's code (abi.ERR_BAD_DESC for a bad request list)."""
    _measure_device("spicey_power_device", (n_inst, n_points, dt), d_v, n_v, d_i, n_i, _reqs(reqs, abi.POWER_REQ_DTYPE), d_out, d_work, work_bytes, device, stream)


def values_workspace_bytes(n_inst: int, n_points: int, reqs, n_pts: int = 0) -> int:
    """spicey_values_workspace_bytes: device workspace of values_device for this request list and a point table of n_pts
    records; -1 for a refused one."""
    r = _reqs(reqs, abi.VAL_REQ_DTYPE)
    return load().spicey_values_workspace_bytes(n_inst, n_points, _reqs_ptr(r), len(r), n_pts)


def values_device(n_inst: int, n_points: int, dt: float, d_v: int, n_v: int, d_i: int, n_i: int, reqs, pts, d_timing: int, n_timing: int, d_out: int,
                  out_stride: int, d_work: int, work_bytes: int, device: int = 0, stream: int = 0) -> None:
    """spicey_values_device: the values pass alone on raw device pointers (e.g. torch tensors' data_ptr()): d_v
    [n_inst][n_points][n_v], d_i [n_inst][n_points][n_i] or 0, d_timing [n_inst][n_timing][8] (a timing pass's rows) or 0, d_out
    [n_inst][n_req][out_stride], d_work of `work_bytes` >= values_workspace_bytes(...).  reqs: records of abi.VAL_REQ_DTYPE;
    pts: records of abi.VAL_POINT_DTYPE (host; may be empty).  Enqueued on `stream`, no synchronisation.  A refusal raises
    SpiceyNativeError whose `status` is the library's code (abi.ERR_BAD_DESC for a bad request list)."""
    L = load()
    r = _reqs(reqs, abi.VAL_REQ_DTYPE)
    pt = _reqs(pts if len(pts) else [], abi.VAL_POINT_DTYPE)
    rc = L.spicey_values_device(device, n_inst, n_points, dt, d_v or None, n_v, d_i or None, n_i, _reqs_ptr(r), len(r), _reqs_ptr(pt), len(pt),
                                d_timing or None, n_timing, d_out or None, out_stride, d_work or None, work_bytes, stream or None)
    if rc != abi.OK:
        _fail("spicey_values_device", rc, L.spicey_last_error(None))


# The reduction passes behind a transient run, in the order they run: result key, list and count field of abi.SpiceyReducedLists,
# record dtype, doubles of a result row (a number, or the rule over the list's records), key and function of the pass's time.
_PASSES = (
    ("meas", "reqs", "n_req", abi.MEAS_REQ_DTYPE, 8, "measure_ms", "spicey_last_measure_ms"),
    ("four", "freqs", "n_four", abi.FOUR_REQ_DTYPE, fourier_row_doubles, "fourier_ms", "spicey_last_fourier_ms"),
    ("timing", "treqs", "n_timing", abi.TIMING_REQ_DTYPE, 8, "timing_ms", "spicey_last_timing_ms"),
    ("spec", "sreqs", "n_spec", abi.SPEC_REQ_DTYPE, abi.spec_row_doubles, "spectrum_ms", "spicey_last_spectrum_ms"),
    ("power", "preqs", "n_power", abi.POWER_REQ_DTYPE, abi.POWER_ROW, "power_ms", "spicey_last_power_ms"),
    ("values", "vreqs", "n_values", abi.VAL_REQ_DTYPE, abi.val_row_doubles, "values_ms", "spicey_last_values_ms"),
)
_PASS_MS = tuple(p[5:] for p in _PASSES)
_MC_MS = (("mc_ms", "spicey_last_tran_mc_ms"), ("draw_ms", "spicey_last_tran_mc_draw_ms"))
_SENS_MS = (("sens_ms", "spicey_last_tran_sens_ms"), ("design_ms", "spicey_last_tran_sens_design_ms"))


def _pass_list(r, dtype, row):
    """A pass's request list as records of `dtype`, and the doubles of its result row."""
    r = _reqs(r if len(r) else [], dtype)
    return r, row(r) if callable(row) else row


class Handle:
    """Owns one SpiceyHandle (one topology, n_inst instances, one device)."""

    def __init__(self, flat: abi.FlatCircuit, device: int = 0, threads: int = 0, inst_per_wg: int = 0,
                 force_global: bool = False, profile: bool = False, interpreter: int = 0, geometry: int = 0, no_tail: bool = False, debug_empty_phases: int = 0, wgs_per_inst: int = 0,
                 no_reuse: bool = False, csr_numbering: bool = False, front_cut: int = 0, stage_fronts: bool = False, no_pcr: bool = False, no_rows: bool = False,
                 group_retry: bool = False, group_timeout_ms: int = 0, diagnostics: int = 0):
        self.L = load()
        self.flat = flat
        opt = abi.SpiceyOptions()
        opt.device, opt.threads, opt.inst_per_wg, opt.want_currents, opt.force_global = device, threads, inst_per_wg, 1, int(force_global)
        opt.profile = int(profile)
        opt.interpreter = int(interpreter)
        opt.geometry = int(geometry)
        opt.wgs_per_inst = int(wgs_per_inst)
        opt.front_cut = int(front_cut)
        opt.group_retry, opt.group_timeout_ms, opt.diagnostics = int(group_retry), int(group_timeout_ms), int(diagnostics)
        self.diagnostics = int(diagnostics)
        opt.debug = (1 if no_tail else 0) | (2 if no_reuse else 0) | (4 if csr_numbering else 0) | (8 if stage_fronts else 0) | (32 if no_pcr else 0) | (64 if no_rows else 0) | (int(debug_empty_phases) << 8)
        d = flat.desc()
        hp = C.c_void_p()
        rc = self.L.spicey_create(C.byref(d), C.byref(opt), C.byref(hp))
        if rc != abi.OK:
            _fail("spicey_create", rc, self.L.spicey_last_error(None))
        self.h = hp

    def info(self) -> dict:
        i = abi.SpiceyInfo()
        self.L.spicey_get_info(self.h, C.byref(i))
        return i.as_dict()

    def top_regs_form(self, steps: int) -> bool:
        """Whether a run of `steps` steps takes the kernel with the register-exchange top (spicey_top_regs_form)."""
        return bool(self.L.spicey_top_regs_form(self.h, steps))

    def u0_resident_form(self, steps: int) -> bool:
        """Whether a run of `steps` steps takes the kernel that keeps level 0's row record in registers (spicey_u0_resident_form)."""
        return bool(self.L.spicey_u0_resident_form(self.h, steps))

    def top_fold_form(self, steps: int) -> bool:
        """Whether a run of `steps` steps takes the kernel whose top runs the last factor level itself (spicey_top_fold_form)."""
        return bool(self.L.spicey_top_fold_form(self.h, steps))

    def stamp_fuse_form(self, steps: int) -> bool:
        """Whether a run of `steps` steps takes the kernel whose Z stamps the next step, with no phase B in the loop (spicey_stamp_fuse_form)."""
        return bool(self.L.spicey_stamp_fuse_form(self.h, steps))

    def fixed_schedule_form(self, steps: int) -> bool:
        """Whether a run of `steps` steps takes the fused kernel whose time loop is written out for the plan (spicey_fixed_schedule_form)."""
        return bool(self.L.spicey_fixed_schedule_form(self.h, steps))

    def error(self) -> str:
        m = self.L.spicey_last_error(self.h)
        return m.decode() if m else ""

    def run(self, steps: int, dt: float, src: np.ndarray, want_currents: bool = True, want_iters: bool = True) -> dict:
        """src: [steps+1][nV], shared by every instance (spicey_run), or [n_inst][steps+1][nV], one table per instance
        (spicey_run_src).  The result carries `inst_status` (spicey_last_inst_status); with per-instance tables it is
        `partial` = True, and after a singular run out_v / out_i / iters / state then hold the instances that finished."""
        f = self.flat
        src = np.ascontiguousarray(src, dtype=np.float64)
        per_inst = _src_layout(src, f, steps)
        out_v = np.empty((f.n_inst, steps + 1, f.n_out))
        out_i = np.empty((f.n_inst, steps + 1, f.n_cur)) if want_currents else None
        iters = np.zeros((f.n_inst, steps + 1), np.int32) if want_iters else None
        if per_inst:
            rc = self.L.spicey_run_src(self.h, steps, dt, _p(src, C.c_double), 1, _p(out_v, C.c_double), _p(out_i, C.c_double),
                                       _p(iters, C.c_int32))
        else:
            rc = self.L.spicey_run(self.h, steps, dt, _p(src, C.c_double), _p(out_v, C.c_double), _p(out_i, C.c_double),
                                   _p(iters, C.c_int32))
        res = {"status": rc, "detail": self.error() if rc != abi.OK else "", "out_v": out_v, "out_i": out_i, "iters": iters,
               "partial": per_inst}
        # (after a singular run with per-instance tables, the instances that finished keep everything a success reports:
        # results, end state and their diagnostics)
        return self._dress(res, rc, rc == abi.OK, rc == abi.OK or (per_inst and rc == abi.ERR_SINGULAR), steps)

    def _dress(self, res: dict, rc: int, timed: bool, kept: bool, lin_err_steps: Optional[int] = None) -> dict:
        """What every transient result carries besides its buffers: `inst_status`; when `timed`, `solves` and `kernel_ms`;
        when `kept` (the run's results stand), the end `state` and the diagnostics this handle was opened with."""
        f = self.flat
        res["inst_status"] = self.inst_status() if rc in (abi.OK, abi.ERR_SINGULAR) else np.full(f.n_inst, rc, np.int32)
        if timed:
            res["solves"] = self.L.spicey_last_solve_count(self.h)
            res["kernel_ms"] = self.L.spicey_last_kernel_ms(self.h)
        if kept:
            res["state"] = self.state()
            if self.diagnostics & 1:
                per = np.zeros(f.n_inst, np.int64)
                self.L.spicey_last_skip_risk(self.h, _p(per, C.c_int64))
                res["skip_risk"] = per
            if self.diagnostics & 2 and lin_err_steps is not None:
                le = np.zeros((f.n_inst, lin_err_steps + 1))
                if self.L.spicey_get_lin_err(self.h, _p(le, C.c_double)) != abi.OK:
                    raise SpiceyNativeError(f"spicey_get_lin_err failed: {self.error()}")
                res["lin_err"] = le
        return res

    def _reduced_lists(self, reqs, freqs, treqs, sreqs, preqs, vreqs, pts=(), outs=None, struct_bytes=None):
        """(the filled abi.SpiceyReducedLists, the arrays to keep alive, the row lengths by result key).  outs: None (a study takes no
        result pointers), or the dict that gets one zeroed result array per list, which the struct points to where the list is not
        empty."""
        a = abi.SpiceyReducedLists()
        a.struct_bytes = C.sizeof(a) if struct_bytes is None else struct_bytes
        keep, rows = {"pts": _reqs(pts if len(pts) else [], abi.VAL_POINT_DTYPE)}, {}
        for (key, lst, cnt, dtype, row, _, _), r in zip(_PASSES, (reqs, freqs, treqs, sreqs, preqs, vreqs)):
            keep[key], rows[key] = _pass_list(r, dtype, row)
            setattr(a, lst, _reqs_ptr(keep[key]))
            setattr(a, cnt, len(keep[key]))
            if outs is not None:
                outs[key] = np.zeros((self.flat.n_inst, len(keep[key]), rows[key]))
                setattr(a, key, outs[key].ctypes.data if len(keep[key]) else None)
        a.four_stride, a.spec_stride, a.values_stride = rows["four"], rows["spec"], rows["values"]
        a.pts, a.n_pts = _reqs_ptr(keep["pts"]), len(keep["pts"])
        return a, keep, rows

    def _prologue(self, steps: int, src: np.ndarray, want_iters: bool):
        """What every reduced run starts from: (src as one contiguous array, src_per_inst, the iters array or None)."""
        src = np.ascontiguousarray(src, dtype=np.float64)
        per_inst = _src_layout(src, self.flat, steps)
        return src, 1 if per_inst else 0, np.zeros((self.flat.n_inst, steps + 1), np.int32) if want_iters else None

    def _epilogue(self, res: dict, rc: int, iters, ms) -> dict:
        """What every reduced run ends with: status, detail, iters and `partial` into res; after a run that was kept (OK or
        singular) the time readouts `ms` ((result key, function), ...); the dressing."""
        res.update(status=rc, detail=self.error() if rc != abi.OK else "", iters=iters, partial=True)
        kept = rc in (abi.OK, abi.ERR_SINGULAR)
        if kept:
            for key, fn in ms:
                res[key] = getattr(self.L, fn)(self.h)
        return self._dress(res, rc, kept, kept)

    def _run_reduced(self, entry: int, steps: int, dt: float, src: np.ndarray, reqs, freqs, treqs, want_iters: bool, sreqs=None, preqs=None) -> dict:
        """What run_measure (entry 0), run_measure_fourier (1), run_measure_timing (2), run_measure_spectrum (3) and
        run_measure_power (4) share: the result arrays of the passes that entry has — an empty list of an earlier pass goes
        down as a null out pointer — its C function, and the dressing."""
        src, per_inst, iters = self._prologue(steps, src, want_iters)
        res = {"status": 0, "detail": ""}
        args, keep = [], []
        lists = (reqs, freqs, treqs, [] if sreqs is None else sreqs, [] if preqs is None else preqs)
        for k, ((key, _, _, dtype, row, _, _), r) in enumerate(zip(_PASSES[:entry + 1], lists)):
            r, n_row = _pass_list(r, dtype, row)
            keep.append(r)
            res[key] = np.zeros((self.flat.n_inst, len(r), n_row))
            args += [_reqs_ptr(r), len(r), _p(res[key], C.c_double) if len(r) or k == entry else None]
            if callable(row):
                args.append(n_row)
        fn = (self.L.spicey_run_measure, self.L.spicey_run_measure_fourier, self.L.spicey_run_measure_timing, self.L.spicey_run_measure_spectrum,
              self.L.spicey_run_measure_power)[entry]
        rc = fn(self.h, steps, dt, _p(src, C.c_double), per_inst, *args, _p(iters, C.c_int32))
        return self._epilogue(res, rc, iters, _PASS_MS[:entry + 1])

    def run_measure(self, steps: int, dt: float, src: np.ndarray, reqs, want_iters: bool = True) -> dict:
        """spicey_run_measure: the transient with its waveforms kept on the device and reduced there; only `meas`
        [n_inst][n_req][8] (include/spicey_hip.h) and the iteration counts come back.  reqs: records of abi.MEAS_REQ_DTYPE
        (spicey_amd/measure.py), columns as in this handle's out_v / out_i.  Like run() with per-instance tables, the rows of
        the instances that finished are also there after a singular run (`inst_status`); `partial` says so."""
        return self._run_reduced(0, steps, dt, src, reqs, [], [], want_iters)

    def run_measure_fourier(self, steps: int, dt: float, src: np.ndarray, reqs, freqs, want_iters: bool = True) -> dict:
        """spicey_run_measure_fourier: run_measure with the harmonics pass behind the measurements, over the same device
        waveforms.  reqs: records of abi.MEAS_REQ_DTYPE (may be empty), freqs: records of abi.FOUR_REQ_DTYPE (at least one).
        Beside what run_measure returns: `four` [n_inst][n_four][1 + 2 max n_harm] = {C0, C1, S1, ...} per request, the rest
        of a row 0 (include/spicey_hip.h), and `fourier_ms`."""
        return self._run_reduced(1, steps, dt, src, reqs, freqs, [], want_iters)

    def run_measure_timing(self, steps: int, dt: float, src: np.ndarray, reqs, freqs, treqs, want_iters: bool = True) -> dict:
        """spicey_run_measure_timing: run_measure_fourier with the edge-timing pass behind the other two, over the same device
        waveforms.  reqs: records of abi.MEAS_REQ_DTYPE (may be empty), freqs: records of abi.FOUR_REQ_DTYPE (may be empty),
        treqs: records of abi.TIMING_REQ_DTYPE (at least one).  Beside what run_measure_fourier returns: `timing`
        [n_inst][n_timing][8] = {k_trig, t_trig, L_trig, k_targ, t_targ, L_targ, n_trig, n_targ} (include/spicey_hip.h) and
        `timing_ms`."""
        return self._run_reduced(2, steps, dt, src, reqs, freqs, treqs, want_iters)

    def run_measure_spectrum(self, steps: int, dt: float, src: np.ndarray, reqs, freqs, treqs, sreqs, want_iters: bool = True) -> dict:
        """spicey_run_measure_spectrum: run_measure_timing with the spectrum pass behind the other three, over the same device
        waveforms.  reqs, freqs, treqs: as for run_measure_timing, each may be empty; sreqs: records of abi.SPEC_REQ_DTYPE (at
        least one).  Beside what run_measure_timing returns: `spec` [n_inst][n_spec][row] — per request {re, im} of the band's
        bins or {k, re_k, im_k, P_k-1, P_k, P_k+1, 0, 0}, the rest of a row 0 (include/spicey_hip.h) — and `spectrum_ms`."""
        return self._run_reduced(3, steps, dt, src, reqs, freqs, treqs, want_iters, sreqs)

    def run_measure_power(self, steps: int, dt: float, src: np.ndarray, reqs, freqs, treqs, sreqs, preqs, want_iters: bool = True) -> dict:
        """spicey_run_measure_power: run_measure_spectrum with the product pass behind the other four, over the same device
        waveforms.  reqs, freqs, treqs, sreqs: as for run_measure_spectrum, each may be empty; preqs: records of
        abi.POWER_REQ_DTYPE (at least one).  Beside what run_measure_spectrum returns: `power` [n_inst][n_power][abi.POWER_ROW] =
        {min_p, max_p, step_min, step_max, sum_p, first_p, last_p, sum_aa, sum_bb, first_a, last_a, first_b, last_b, 0, 0, 0}
        (include/spicey_hip.h) and `power_ms`."""
        return self._run_reduced(4, steps, dt, src, reqs, freqs, treqs, want_iters, sreqs, preqs)

    def run_reduced(self, steps: int, dt: float, src: np.ndarray, reqs=(), freqs=(), treqs=(), sreqs=(), preqs=(), vreqs=(), pts=(),
                    want_iters: bool = True, struct_bytes: Optional[int] = None) -> dict:
        """spicey_run_reduced: one transient run and, over the same device waveforms, every pass whose list is not empty —
        measurement, harmonics, timing, spectrum, products, values — through one struct (abi.SpiceyReducedLists) instead of one
        positional entry point per pass.  The lists are as for run_measure_power; vreqs: records of abi.VAL_REQ_DTYPE, pts:
        their point table (abi.VAL_POINT_DTYPE); a find request's timing_row indexes treqs.  Returns what run_measure_power
        returns for the passes that ran (`meas`, `four`, `timing`, `spec`, `power` are there for every list, [n_inst][0][row]
        for an empty one) plus `values` [n_inst][n_values][abi.val_row_doubles(vreqs)] and `values_ms`.  struct_bytes: the
        size the struct claims (tests)."""
        src, per_inst, iters = self._prologue(steps, src, want_iters)
        res = {"status": 0, "detail": ""}
        a, keep, _ = self._reduced_lists(reqs, freqs, treqs, sreqs, preqs, vreqs, pts, res, struct_bytes)
        rc = self.L.spicey_run_reduced(self.h, steps, dt, _p(src, C.c_double), per_inst, C.byref(a), _p(iters, C.c_int32))
        del keep
        return self._epilogue(res, rc, iters, _PASS_MS)

    def run_mc(self, steps: int, dt: float, src: np.ndarray, req: abi.SpiceyTranMcReq, tol, icdf, scalars, lo=None, hi=None, probs=(), reqs=(), treqs=(),
               preqs=(), freqs=(), sreqs=(), vreqs=(), want_x: bool = False, want_iters: bool = False) -> dict:
        """spicey_run_mc: the handle's instances are the samples, its value rows their nominal values; R, C and L are drawn on the
        device, ONE transient reads them, the measure / timing / power passes of reqs / treqs / preqs run behind it and stay on
        the device, and `scalars` (records of abi.MC_SCALAR_DTYPE over those rows) are reduced across the samples.  tol [nE]
        (out_i's column order: R, C, L), icdf [2^log2K + 1], lo / hi [n_scalar] (None: no limit) and probs are host arrays.
        Returns `stat` [n_scalar][8 + 2 n_prob] and `sample` [n_inst][2] (include/spicey_hip.h), `x` [n_inst][n_scalar] with
        want_x, `inst_status`, `state`, `mc_ms`, `draw_ms`.  freqs / sreqs / vreqs are there to be refused."""
        f = self.flat
        src, per_inst, iters = self._prologue(steps, src, want_iters)
        a, keep, _ = self._reduced_lists(reqs, freqs, treqs, sreqs, preqs, vreqs)
        sc = _scalars(scalars)
        t, tab = _host(tol, np.float64), _host(icdf, np.float64)
        lo_, hi_, pr = _host(lo, np.float64), _host(hi, np.float64), np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        stat = np.zeros((len(sc), abi.TRAN_MC_STAT_HEAD + 2 * len(pr)))
        sample = np.full((f.n_inst, 2), -1, np.int64)
        x = np.full((f.n_inst, len(sc)), np.nan) if want_x else None
        rc = self.L.spicey_run_mc(self.h, steps, dt, _p(src, C.c_double), per_inst, C.addressof(a), C.addressof(req) if req is not None else None,
                                  _p(t, C.c_double), _p(tab, C.c_double), sc.ctypes.data if len(sc) else None, len(sc), _p(lo_, C.c_double), _p(hi_, C.c_double),
                                  _p(pr, C.c_double) if len(pr) else None, len(pr), _p(stat, C.c_double), _p(sample, C.c_int64), _p(x, C.c_double),
                                  _p(iters, C.c_int32))
        del keep
        return self._epilogue({"status": 0, "detail": "", "stat": stat, "sample": sample, "x": x}, rc, iters, _MC_MS)

    def run_sens(self, steps: int, dt: float, src: np.ndarray, req: abi.SpiceyTranSensReq, act, step, tol, scalars, reqs=(), treqs=(), preqs=(), freqs=(), sreqs=(),
                 vreqs=(), want_x: bool = False, want_iters: bool = False) -> dict:
        """spicey_run_sens: the handle's n_inst = 1 + 2 nA instances are the nominal circuit and, per active element act[a], the
        variants with that element at 1 + step[a] and 1 - step[a] times its value; the design is written on the device, ONE
        transient reads it, the measure / timing / power passes run behind it and stay on the device, and `scalars` are reduced
        across the instances.  act [nA] (int32), step [nA], tol [nE] (order R, C, L) are host arrays.  Returns `sens`
        [n_scalar][nA][2] = {d, c}, `sign` [n_scalar][nA] int8, `bound` [n_scalar][8] (include/spicey_hip.h), `x`
        [n_inst][n_scalar] with want_x, `inst_status`, `state`, `sens_ms`, `design_ms`.  freqs / sreqs / vreqs are there to be refused."""
        f = self.flat
        src, per_inst, iters = self._prologue(steps, src, want_iters)
        a, keep, _ = self._reduced_lists(reqs, freqs, treqs, sreqs, preqs, vreqs)
        sc = _scalars(scalars)
        ac, st, tl = _host(act, np.int32), _host(step, np.float64), _host(tol, np.float64)
        nA = int(req.nA) if req is not None else 0
        sens = np.full((len(sc), max(nA, 0), 2), np.nan)
        sign = np.zeros((len(sc), max(nA, 0)), np.int8)
        bound = np.zeros((len(sc), abi.TRAN_SENS_BOUND_ROW))
        x = np.full((f.n_inst, len(sc)), np.nan) if want_x else None
        rc = self.L.spicey_run_sens(self.h, steps, dt, _p(src, C.c_double), per_inst, C.addressof(a), C.addressof(req) if req is not None else None,
                                    _data(ac), _p(st, C.c_double), _p(tl, C.c_double), sc.ctypes.data if len(sc) else None, len(sc), _p(sens, C.c_double),
                                    sign.ctypes.data, _p(bound, C.c_double), _p(x, C.c_double), _p(iters, C.c_int32))
        del keep
        return self._epilogue({"status": 0, "detail": "", "sens": sens, "sign": sign, "bound": bound, "x": x}, rc, iters, _SENS_MS)

    def run_levels(self, steps: int, dt: float, src: np.ndarray, req: abi.SpiceyTranSensReq, lvl, tol, scalars, reqs=(), treqs=(), preqs=(), freqs=(), sreqs=(),
                   vreqs=(), want_iters: bool = False) -> dict:
        """spicey_run_levels: run_sens with the LEVELS design — instance s has element e at 1 + lvl[s][e] tol[e] times its value,
        lvl [n_inst][nE] int8 in {-1, 0, +1} — and no reduction: returns `x` [n_inst][n_scalar], NaN for an invalid instance."""
        src, per_inst, iters = self._prologue(steps, src, want_iters)
        a, keep, _ = self._reduced_lists(reqs, freqs, treqs, sreqs, preqs, vreqs)
        sc = _scalars(scalars)
        lv, tl = _host(lvl, np.int8), _host(tol, np.float64)
        x = np.full((self.flat.n_inst, len(sc)), np.nan)
        rc = self.L.spicey_run_levels(self.h, steps, dt, _p(src, C.c_double), per_inst, C.addressof(a), C.addressof(req) if req is not None else None,
                                      _data(lv), _p(tl, C.c_double), sc.ctypes.data if len(sc) else None, len(sc), _p(x, C.c_double), _p(iters, C.c_int32))
        del keep
        return self._epilogue({"status": 0, "detail": "", "x": x}, rc, iters, _SENS_MS)

    def run_pss(self, m_steps: int, dt: float, src: np.ndarray, req: abi.SpiceyPssReq) -> dict:
        """spicey_run_pss: the shooting-Newton loop on this handle, whose n_inst = req.n_ckt W instances are the circuits' nominal and
        perturbed copies; src holds the m_steps source rows of one period, [m_steps][nV] or [n_inst][m_steps][nV].  Returns `x`
        [n_ckt][nX] and `on` [n_ckt][nS] (the base on return), `history` [iterations][n_ckt][8], `n_iter` and `ckt_status` [n_ckt]
        (include/spicey_hip.h), `inst_status` of the last transient, `pss_ms` (designs and updates) and `tran_ms` (the transients'
        kernels), summed over the iterations.  A refusal comes back as status abi.ERR_BAD_DESC with its text in `detail`."""
        f = self.flat
        src = np.ascontiguousarray(src, dtype=np.float64)
        per_inst = _src_layout(src, f, m_steps - 1) if m_steps >= 1 else False
        n_ckt, max_iter = max(int(req.n_ckt), 0) if req is not None else 0, max(int(req.max_iter), 0) if req is not None else 0
        x = np.zeros((n_ckt, f.nC + f.nL + f.nD))
        on = np.zeros((n_ckt, f.nS), np.int32)
        history = np.zeros((max_iter, n_ckt, abi.PSS_ROW))
        n_iter, st = np.zeros(max(n_ckt, 1), np.int32), np.ones(max(n_ckt, 1), np.int32)
        rc = self.L.spicey_run_pss(self.h, m_steps, dt, _p(src, C.c_double), 1 if per_inst else 0, C.addressof(req) if req is not None else None, _p(x, C.c_double),
                                   _p(on, C.c_int32), _p(history, C.c_double), _p(n_iter, C.c_int32), _p(st, C.c_int32))
        res = {"status": rc, "detail": self.error(), "x": x, "on": on, "n_iter": n_iter[:n_ckt], "ckt_status": st[:n_ckt],
               "history": history[:int(n_iter[:n_ckt].max()) if n_ckt else 0]}
        if rc == abi.OK:
            res["pss_ms"], res["tran_ms"] = self.L.spicey_last_pss_ms(self.h), self.L.spicey_last_pss_tran_ms(self.h)
            try:
                res["inst_status"] = self.inst_status()
            except SpiceyNativeError:
                res["inst_status"] = None  # (no transient ran)
        return res

    def run_fit(self, steps: int, dt: float, src: np.ndarray, req: abi.SpiceyFitReq, act, step, g_lo, g_hi, g0, goals, scalars, reqs=(), treqs=(), preqs=(),
                freqs=(), sreqs=(), vreqs=(), want_iters: bool = False) -> dict:
        """spicey_run_fit: the damped least-squares loop on this handle, whose n_inst = req.n_ckt (1 + 2 nA) instances are the
        circuits' nominal and perturbed copies.  act [nA] (int32), step [nA], g_lo / g_hi / g0 [n_ckt][nA], goals [n_ckt][n_scalar]
        (abi.FIT_GOAL_DTYPE) are host arrays, scalars the programs of abi.MC_SCALAR_DTYPE over the rows of reqs / treqs / preqs.
        Returns `g` [n_ckt][nA] and `F` [n_ckt] (the best evaluated point), `x` [n_ckt][n_scalar] (the nominals' scalars there),
        `history` [iterations][n_ckt][8], `n_iter` and `ckt_status` [n_ckt] (include/spicey_hip.h), `inst_status` of the last
        transient, `fit_ms` (designs and updates) and `tran_ms` (the transients' kernels), summed over the iterations.  A refusal
        comes back as status abi.ERR_BAD_DESC with its text in `detail`.  freqs / sreqs / vreqs are there to be refused."""
        src, per_inst, iters = self._prologue(steps, src, want_iters)
        a, keep, _ = self._reduced_lists(reqs, freqs, treqs, sreqs, preqs, vreqs)
        sc = _scalars(scalars)
        ac, st = _host(act, np.int32), _host(step, np.float64)
        lo, hi, g0_, go = _host(g_lo, np.float64), _host(g_hi, np.float64), _host(g0, np.float64), _goals(goals)
        n_ckt, nA = (max(int(req.n_ckt), 0), max(int(req.nA), 0)) if req is not None else (0, 0)
        max_iter = max(int(req.max_iter), 0) if req is not None else 0
        g, F = np.zeros((n_ckt, nA)), np.full(max(n_ckt, 1), np.inf)
        x = np.full((n_ckt, len(sc)), np.nan)
        history = np.zeros((max_iter, n_ckt, abi.FIT_ROW))
        n_iter, cst = np.zeros(max(n_ckt, 1), np.int32), np.ones(max(n_ckt, 1), np.int32)
        rc = self.L.spicey_run_fit(self.h, steps, dt, _p(src, C.c_double), per_inst, C.addressof(a), C.addressof(req) if req is not None else None, _data(ac),
                                   _p(st, C.c_double), _p(lo, C.c_double), _p(hi, C.c_double), _p(g0_, C.c_double), _data(go), sc.ctypes.data if len(sc) else None,
                                   len(sc), _p(g, C.c_double), _p(F, C.c_double), _p(history, C.c_double), _p(n_iter, C.c_int32), _p(cst, C.c_int32),
                                   _p(x, C.c_double), _p(iters, C.c_int32))
        del keep
        res = {"status": rc, "detail": self.error() if rc != abi.OK else "", "g": g, "F": F[:n_ckt], "x": x, "n_iter": n_iter[:n_ckt], "ckt_status": cst[:n_ckt],
               "history": history[:int(n_iter[:n_ckt].max()) if n_ckt else 0], "iters": iters}
        if rc == abi.OK:
            res["fit_ms"], res["tran_ms"] = self.L.spicey_last_fit_ms(self.h), self.L.spicey_last_fit_tran_ms(self.h)
            try:
                res["inst_status"] = self.inst_status()
            except SpiceyNativeError:
                res["inst_status"] = None  # (no transient ran)
        return res

    def run_device(self, steps: int, dt: float, d_src: int, d_out_v: int, d_out_i: int = 0, d_iters: int = 0, stream: int = 0,
                   src_per_inst: bool = False) -> None:
        """Enqueue with raw device pointers (e.g. torch tensors' data_ptr()); no synchronisation.  src_per_inst: d_src holds
        [n_inst][steps+1][nV] (spicey_run_device_src) instead of one shared [steps+1][nV] table."""
        if src_per_inst:
            rc = self.L.spicey_run_device_src(self.h, steps, dt, d_src, 1, d_out_v, d_out_i or None, d_iters or None, stream or None)
        else:
            rc = self.L.spicey_run_device(self.h, steps, dt, d_src, d_out_v, d_out_i or None, d_iters or None, stream or None)
        if rc != abi.OK:
            _fail("spicey_run_device", rc, self.error())

    def inst_status(self) -> np.ndarray:
        """Per instance of the last run (spicey_last_inst_status): 0 finished, 1 = SPICEY_ERR_SINGULAR (its own solve), -1 =
        stopped because another instance of its workgroup failed, 3 = the launch aborted."""
        st = np.zeros(self.flat.n_inst, np.int32)
        if self.L.spicey_last_inst_status(self.h, _p(st, C.c_int32)) < 0:
            raise SpiceyNativeError(f"spicey_last_inst_status failed: {self.error()}")
        return st

    def sync(self) -> int:
        return self.L.spicey_sync(self.h)

    def solves(self) -> int:
        return self.L.spicey_last_solve_count(self.h)

    def front_ticks(self, grp: int = 0):
        """(ticks[nf][4] uint64 summed over the solves, meta[nf][4] = pivots, boundary, parent, owner) of the last run
        (profile=True, circuits with dense fronts); include/spicey_hip.h, spicey_debug_front_ticks."""
        nf = self.info()["n_fronts"]
        t = np.zeros((max(nf, 1), 4), np.uint64)
        m = np.zeros((max(nf, 1), 4), np.int32)
        got = self.L.spicey_debug_front_ticks(self.h, grp, t.ctypes.data_as(C.POINTER(C.c_uint64)), m.ctypes.data_as(C.POINTER(C.c_int32)), nf)
        return t[:got], m[:got]

    def group_retries(self) -> int:
        """Group-mode launches this handle repeated after a bounded-spin abort (include/spicey_hip.h, spicey_sync)."""
        return self.L.spicey_group_retries(self.h)

    def group_stale_polls(self) -> int:
        """Group mode: waits of this handle's launches that only the read-modify-write poll saw satisfied (0 when healthy)."""
        return self.L.spicey_group_stale_polls(self.h)

    def kernel_ms(self) -> float:
        return self.L.spicey_last_kernel_ms(self.h)

    def phase_cycles(self) -> dict:
        """Shader-clock cycles per phase kind of workgroup 0 in the last run (needs profile=True)."""
        buf = (C.c_uint64 * 72)()
        self.L.spicey_debug_phase_cycles(self.h, buf, 72)
        a = list(buf)
        return {"prologue": a[0], "B": a[1], "S": a[2], "A": a[3], "Z": a[4], "run_cycles": a[5], "run_wall_ticks_100MHz": a[6], "between_phases": a[7],
                "U": a[8:40], "K": a[40:72]}

    def section_ticks(self, wg: int) -> list:
        """Group mode, profile=True: 100 MHz wall ticks per section of launched workgroup `wg` (see spicey_hip.h)."""
        buf = (C.c_uint64 * 72)()
        self.L.spicey_debug_phase_cycles_wg(self.h, int(wg), buf, 72)
        return list(buf)

    def state(self) -> dict:
        st, ptrs = _state_arrays(self.flat)
        rc = self.L.spicey_get_state(self.h, *ptrs)
        if rc != abi.OK:
            _fail("spicey_get_state", rc, self.error())
        return st

    def set_state(self, st: dict) -> None:
        """State entering the next run: any of C_vprev / L_iprev / D_vdprev [n_inst][n] float64, S_ison int32."""
        a = {k: (np.ascontiguousarray(st[k], dtype=np.int32 if k == "S_ison" else np.float64) if st.get(k) is not None else None)
             for k in ("C_vprev", "L_iprev", "D_vdprev", "S_ison")}
        rc = self.L.spicey_set_state(self.h, _p(a["C_vprev"], C.c_double), _p(a["L_iprev"], C.c_double), _p(a["D_vdprev"], C.c_double),
                                     _p(a["S_ison"], C.c_int32))
        if rc != abi.OK:
            _fail("spicey_set_state", rc, self.error())

    def reset_state(self, stream: int = 0) -> None:
        """Back to the state the handle was created with (device-to-device, enqueued on `stream`)."""
        rc = self.L.spicey_reset_state(self.h, stream or None)
        if rc != abi.OK:
            _fail("spicey_reset_state", rc, self.error())

    def close(self) -> None:
        if getattr(self, "h", None):
            GROUP_TOTALS["retries"] += self.L.spicey_group_retries(self.h)
            GROUP_TOTALS["stale_polls"] += self.L.spicey_group_stale_polls(self.h)
            self.L.spicey_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiHandle:
    """spicey_create_multi / spicey_run_multi: the instances of one FlatCircuit block-partitioned over several devices
    inside this process, results gathered into one host buffer (SURVEY.md §8(b) "device ordinal(s)", §8(e))."""

    def __init__(self, flat: abi.FlatCircuit, devices, **opts):
        self.L = load()
        self.flat = flat
        opt = abi.SpiceyOptions()
        opt.want_currents = 1
        for k, v in opts.items():
            setattr(opt, k, int(v))
        d = flat.desc()
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        hp = C.c_void_p()
        rc = self.L.spicey_create_multi(C.byref(d), C.byref(opt), _p(devs, C.c_int32) if len(devs) else None, len(devs), C.byref(hp))
        if rc != abi.OK:
            _fail("spicey_create_multi", rc, self.L.spicey_multi_last_error(None))
        self.h = hp

    def shards(self) -> list:
        out = []
        i = 0
        while True:
            info = abi.SpiceyInfo()
            dev, first, cnt = C.c_int32(), C.c_int32(), C.c_int32()
            if self.L.spicey_multi_get_shard(self.h, i, C.byref(info), C.byref(dev), C.byref(first), C.byref(cnt)) != abi.OK:
                return out
            out.append({"device": dev.value, "first_inst": first.value, "n_inst": cnt.value, "info": info.as_dict()})
            i += 1

    def run(self, steps: int, dt: float, src: np.ndarray, want_currents: bool = True, want_iters: bool = True) -> dict:
        """src: [steps+1][nV] shared, or [n_inst][steps+1][nV] per instance (spicey_run_multi_src: each shard its slice)."""
        f = self.flat
        src = np.ascontiguousarray(src, dtype=np.float64)
        per_inst = src.ndim == 3 and _src_layout(src, f, steps)
        out_v = np.empty((f.n_inst, steps + 1, f.n_out))
        out_i = np.empty((f.n_inst, steps + 1, f.n_cur)) if want_currents else None
        iters = np.zeros((f.n_inst, steps + 1), np.int32) if want_iters else None
        if per_inst:
            rc = self.L.spicey_run_multi_src(self.h, steps, dt, _p(src, C.c_double), 1, _p(out_v, C.c_double), _p(out_i, C.c_double),
                                             _p(iters, C.c_int32))
        else:
            rc = self.L.spicey_run_multi(self.h, steps, dt, _p(src, C.c_double), _p(out_v, C.c_double), _p(out_i, C.c_double), _p(iters, C.c_int32))
        detail = self.L.spicey_multi_last_error(self.h).decode() if rc != abi.OK else ""
        res = {"status": rc, "detail": detail, "out_v": out_v, "out_i": out_i, "iters": iters}
        if rc == abi.OK:
            res["state"], ptrs = _state_arrays(f)
            self.L.spicey_get_state_multi(self.h, *ptrs)
            res["solves"] = self.L.spicey_multi_last_solve_count(self.h)
            res["kernel_ms"] = self.L.spicey_multi_last_kernel_ms(self.h)
        return res

    def group_retries(self) -> int:
        return self.L.spicey_multi_group_retries(self.h)

    def group_stale_polls(self) -> int:
        return self.L.spicey_multi_group_stale_polls(self.h)

    def close(self) -> None:
        if getattr(self, "h", None):
            GROUP_TOTALS["retries"] += self.L.spicey_multi_group_retries(self.h)
            GROUP_TOTALS["stale_polls"] += self.L.spicey_multi_group_stale_polls(self.h)
            self.L.spicey_destroy_multi(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_tran_native(times: np.ndarray, values: np.ndarray, cols, header: str) -> str:
    """spicey_format_tran: CSV text of formatTranResult from a [n_points][stride] matrix (host code, multi-threaded)."""
    L = load()
    times = np.ascontiguousarray(times, dtype=np.float64)
    values = np.ascontiguousarray(values, dtype=np.float64)
    if values.ndim != 2 or values.shape[0] != len(times):
        raise ValueError("values must be [n_points][stride]")
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    hdr = header.encode("utf-8")
    need = L.spicey_format_tran(len(times), len(cols), _p(times, C.c_double), _p(values, C.c_double), values.shape[1],
                                _p(cols, C.c_int32), hdr, None, 0)
    if need < 0:
        raise SpiceyNativeError("spicey_format_tran: bad arguments")
    buf = C.create_string_buffer(int(need) + 1)
    L.spicey_format_tran(len(times), len(cols), _p(times, C.c_double), _p(values, C.c_double), values.shape[1],
                         _p(cols, C.c_int32), hdr, buf, need)
    return buf.raw[:need].decode("utf-8")


def to_precision6_native(x: float) -> str:
    buf = C.create_string_buffer(40)
    n = load().spicey_to_precision6(float(x), buf)
    return buf.raw[:n].decode("ascii")


class AcHandle:
    """spicey_ac_* of include/spicey_hip.h: AC sweep of n_inst instances of one topology."""

    def __init__(self, flat: abi.FlatCircuit, device: int = 0, threads: int = 0, force_global: bool = False, no_resident: bool = False, no_dense: bool = False,
                 interpreter: int = 0):
        self.L = load()
        self.flat = flat
        opt = abi.SpiceyOptions()
        opt.device, opt.threads, opt.force_global = int(device), int(threads), int(bool(force_global))
        # interpreter 3: the reference-order engine (the reference's own solveComplex, bit for bit; include/spicey_hip.h)
        opt.interpreter = int(interpreter)
        # bit 4: one workgroup per (instance, frequency) even for large batches; bit 7: no dense partial-pivoting fallback
        opt.debug = (16 if no_resident else 0) | (128 if no_dense else 0)
        d = flat.desc()
        h = C.c_void_p()
        rc = self.L.spicey_ac_create(C.byref(d), C.byref(opt), C.byref(h))
        if rc != abi.OK:
            _fail("spicey_ac_create", rc, self.L.spicey_ac_last_error(None))
        self.h = h

    def info(self) -> dict:
        info = abi.SpiceyInfo()
        self.L.spicey_ac_get_info(self.h, C.byref(info))
        return info.as_dict()

    def _sweep_args(self, freqs, vph):
        """(freqs float64, phasors [n_inst][nV] complex128): one phasor set for every instance, or one per instance."""
        f = self.flat
        return (np.ascontiguousarray(freqs, dtype=np.float64),
                np.ascontiguousarray(np.broadcast_to(np.asarray(vph, np.complex128).reshape(-1, f.nV), (f.n_inst, f.nV))))

    def _dress(self, res: dict, rc: int) -> dict:
        res["status"], res["detail"] = rc, self.L.spicey_ac_last_error(self.h).decode() if rc != abi.OK else ""
        res["kernel_ms"] = self.L.spicey_ac_last_kernel_ms(self.h)
        res["inst_status"], res["first_freq"] = self.inst_status(rc)
        return res

    def run(self, freqs, vph, want_currents: bool = True) -> dict:
        f = self.flat
        freqs, ph = self._sweep_args(freqs, vph)
        ni, nf = f.n_inst, len(freqs)
        out_v = np.zeros((ni, nf, f.n_out), np.complex128)
        out_i = np.zeros((ni, nf, f.nR + f.nC + f.nL + f.nV), np.complex128) if want_currents else None
        rc = self.L.spicey_ac_run(self.h, nf, _p(freqs, C.c_double), _p(ph.view(np.float64), C.c_double),
                                  _p(out_v.view(np.float64), C.c_double), _p(out_i.view(np.float64), C.c_double) if want_currents else None)
        return self._dress({"out_v": out_v, "out_i": out_i}, rc)

    def inst_status(self, rc: int = abi.OK):
        """(status[n_inst], first_freq[n_inst]) of the last sweep (spicey_ac_last_inst_status): per instance 0, or the code of
        its lowest failing frequency index and that index (-1 when fine).  A sweep that was refused before its launch (`rc` is
        that call's status) answers every instance with `rc`."""
        st = np.zeros(self.flat.n_inst, np.int32)
        first = np.full(self.flat.n_inst, -1, np.int64)
        if self.L.spicey_ac_last_inst_status(self.h, _p(st, C.c_int32), _p(first, C.c_int64)) < 0:
            if rc == abi.OK:
                raise SpiceyNativeError("spicey_ac_last_inst_status: no sweep has run on this handle")
            st[:] = rc
        return st, first

    def run_measure(self, freqs, vph, reqs) -> dict:
        """spicey_ac_run_measure: the sweep of run() with its results kept on the device and reduced there; only `meas`
        [n_inst][n_req][8] (include/spicey_hip.h) comes back, also after a failing sweep (`inst_status` names the instances
        whose rows are undefined).  reqs: records of abi.AC_MEAS_REQ_DTYPE, columns as in this handle's out_v / out_i."""
        freqs, ph = self._sweep_args(freqs, vph)
        r = _reqs(reqs, abi.AC_MEAS_REQ_DTYPE)
        meas = np.zeros((self.flat.n_inst, len(r), 8))
        rc = self.L.spicey_ac_run_measure(self.h, len(freqs), _p(freqs, C.c_double), _p(ph.view(np.float64), C.c_double), _reqs_ptr(r), len(r),
                                          _p(meas, C.c_double))
        return self._dress({"meas": meas, "measure_ms": self.L.spicey_ac_last_measure_ms(self.h)}, rc)

    def _phasors_ptr(self, vph):
        if vph is None:
            return None, None
        ph = np.ascontiguousarray(np.broadcast_to(np.asarray(vph, np.complex128).reshape(-1, self.flat.nV), (self.flat.n_inst, self.flat.nV)))
        return ph, _p(ph.view(np.float64), C.c_double)

    def run_inject(self, freqs, vph, node_p: int, node_n: int, amp: complex = 1.0, want_currents: bool = True) -> dict:
        """spicey_ac_run_inject: run() with the current `amp` injected into node_p and drawn from node_n (node ids, 0 =
        ground) at every frequency of every instance.  vph None: every source phasor zero."""
        f = self.flat
        freqs = np.ascontiguousarray(freqs, dtype=np.float64)
        ph, php = self._phasors_ptr(vph)
        ni, nf = f.n_inst, len(freqs)
        out_v = np.zeros((ni, nf, f.n_out), np.complex128)
        out_i = np.zeros((ni, nf, f.nR + f.nC + f.nL + f.nV), np.complex128) if want_currents else None
        inj = abi.ac_inject(node_p, node_n, amp)
        rc = self.L.spicey_ac_run_inject(self.h, nf, _p(freqs, C.c_double), php, C.byref(inj), _p(out_v.view(np.float64), C.c_double),
                                         _p(out_i.view(np.float64), C.c_double) if want_currents else None)
        return self._dress({"out_v": out_v, "out_i": out_i}, rc)

    def run_noise(self, freqs, node_p: int, node_n: int, req: abi.SpiceyAcNoiseReq, vph=None, amp: complex = 1.0) -> dict:
        """spicey_ac_run_noise: the injected sweep of run_inject() with its results kept on the device and reduced there;
        `spec` [n_inst][n_freq][4], `contrib` [n_inst][nR], `total` [n_inst][2] and `gain` [n_inst][n_freq] (complex i(V_in),
        None without an input column) (include/spicey_hip.h) come back, also
        after a failing sweep (`inst_status` names the instances whose rows are undefined).  req: abi.ac_noise_req(...),
        columns as in this handle's out_v / out_i."""
        f = self.flat
        freqs = np.ascontiguousarray(freqs, dtype=np.float64)
        ph, php = self._phasors_ptr(vph)
        spec = np.zeros((f.n_inst, len(freqs), abi.NOISE_SPEC))
        contrib = np.zeros((f.n_inst, f.nR))
        total = np.zeros((f.n_inst, 2))
        gain = np.zeros((f.n_inst, len(freqs)), np.complex128) if req.in_col >= 0 else None
        inj = abi.ac_inject(node_p, node_n, amp)
        rc = self.L.spicey_ac_run_noise(self.h, len(freqs), _p(freqs, C.c_double), php, C.byref(inj), C.byref(req), _p(spec, C.c_double),
                                        _p(contrib, C.c_double), _p(total, C.c_double), _p(gain.view(np.float64), C.c_double) if gain is not None else None)
        return self._dress({"spec": spec, "contrib": contrib, "total": total, "gain": gain, "noise_ms": self.L.spicey_ac_last_noise_ms(self.h)}, rc)

    def run_sens(self, freqs, vph, node_p: int, node_n: int, req: abi.SpiceyAcSensReq, tol, full: bool = False) -> dict:
        """spicey_ac_run_sens: the plain sweep of run() and the sweep of run_inject() with a unit current into (node_p, node_n)
        and every phasor zero, both kept on the device and reduced there; `spec` [n_inst][n_freq][6], `peak` [n_inst][nE][4] and,
        with full, `full` [n_inst][n_freq][nE][2] (include/spicey_hip.h) come back, also after a failing sweep (`inst_status`
        names the instances whose rows are undefined).  req: abi.ac_sens_req(...) with this handle's columns and element
        counts; tol [nE] relative tolerances in the order R, C, L.  `kernel_ms` is the sum of the two sweeps."""
        f = self.flat
        freqs, ph = self._sweep_args(freqs, vph)
        nE = f.nR + f.nC + f.nL
        t = None if tol is None else np.ascontiguousarray(tol, dtype=np.float64).reshape(-1)
        if t is not None and len(t) != nE:
            raise ValueError(f"run_sens: tol must have one entry per element ({nE}), got {len(t)}")
        spec = np.zeros((f.n_inst, len(freqs), abi.SENS_SPEC))
        peak = np.zeros((f.n_inst, nE, abi.SENS_PEAK))
        fl = np.zeros((f.n_inst, len(freqs), nE, 2)) if full else None
        inj = abi.ac_inject(node_p, node_n, 1.0)
        rc = self.L.spicey_ac_run_sens(self.h, len(freqs), _p(freqs, C.c_double), _p(ph.view(np.float64), C.c_double), C.byref(inj), C.byref(req),
                                       _p(t, C.c_double), _p(spec, C.c_double), _p(peak, C.c_double), _p(fl, C.c_double))
        return self._dress({"spec": spec, "peak": peak, "full": fl, "sens_ms": self.L.spicey_ac_last_sens_ms(self.h)}, rc)

    def run_mc(self, freqs, vph, req: abi.SpiceyAcMcReq, tol, icdf, lo=None, hi=None, probs=()) -> dict:
        """spicey_ac_run_mc: this handle's instances are the samples, its rows their nominal values.  The draw writes scratch
        value arrays, one sweep reads them and stays on the device, the reduction across the instances runs behind it;
        `freq_stats` [n_freq][4 + 2 n_prob], `sample` [n_inst][2] int64 and, with req.keep_first, `nominal` [n_freq] (the complex H
        of sample 0) come back (include/spicey_hip.h).  tol [nE] in the order R, C, L; icdf [2^log2K + 1]; lo / hi [n_freq]
        limits of |H|^2 or None; probs the probabilities whose two neighbouring order statistics are wanted."""
        f = self.flat
        freqs, ph = self._sweep_args(freqs, vph)
        nf = len(freqs)
        t, tab, lo_, hi_ = _host(tol, np.float64), _host(icdf, np.float64), _host(lo, np.float64), _host(hi, np.float64)
        pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        for name, a, n in (("tol", t, f.nR + f.nC + f.nL), ("lo", lo_, nf), ("hi", hi_, nf)):
            if a is not None and a.size != n:
                raise ValueError(f"run_mc: {name} must have {n} entries, got {a.size}")
        if tab is not None and req is not None and 0 <= req.log2K <= abi.MC_MAX_LOG2K and tab.size != (1 << req.log2K) + 1:
            raise ValueError(f"run_mc: icdf must have 2^log2K + 1 = {(1 << req.log2K) + 1} entries, got {tab.size}")
        stats = np.zeros((max(nf, 0), abi.MC_FREQ_HEAD + 2 * len(pr)))
        sample = np.zeros((f.n_inst, 2), np.int64)
        nominal = np.zeros(nf, np.complex128) if req is not None and req.keep_first else None
        rc = self.L.spicey_ac_run_mc(self.h, nf, _p(freqs, C.c_double), _p(ph.view(np.float64), C.c_double), C.byref(req) if req is not None else None,
                                     _p(t, C.c_double), _p(tab, C.c_double), _p(lo_, C.c_double), _p(hi_, C.c_double), _p(pr, C.c_double) if len(pr) else None,
                                     len(pr), _p(stats, C.c_double), _p(sample, C.c_int64), _p(nominal.view(np.float64), C.c_double) if nominal is not None else None)
        return self._dress({"freq_stats": stats, "sample": sample, "nominal": nominal, "mc_ms": self.L.spicey_ac_last_mc_ms(self.h),
                            "draw_ms": self.L.spicey_ac_last_mc_draw_ms(self.h)}, rc)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.L.spicey_ac_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _AcCalls:
    """run_ac / run_ac_measure of a backend (`kw`, `info`, `ac_launches`): every call on an AC handle of its own."""

    ac_interpreter = 0  # SpiceyOptions.interpreter of the handles

    def _on_ac_handle(self, flat: abi.FlatCircuit, call) -> dict:
        """call(handle) on an AC handle of its own (one handle = one launch); `info` is the handle's after the sweep."""
        h = AcHandle(flat, interpreter=self.ac_interpreter, **{k: self.kw[k] for k in ("device", "threads", "force_global")})
        self.ac_launches.append(flat.n_inst)
        try:
            res = call(h)
            self.info = h.info()
            return res
        finally:
            h.close()

    def run_ac(self, flat: abi.FlatCircuit, freqs, vph, want_currents: bool = True) -> dict:
        return self._on_ac_handle(flat, lambda h: h.run(freqs, vph, want_currents))

    def run_ac_measure(self, flat: abi.FlatCircuit, freqs, vph, reqs) -> dict:
        """AcHandle.run_measure on a handle of its own: the sweep's results never leave the device."""
        return self._on_ac_handle(flat, lambda h: h.run_measure(freqs, vph, reqs))

    def run_ac_inject(self, flat: abi.FlatCircuit, freqs, vph, node_p: int, node_n: int, amp: complex = 1.0, want_currents: bool = True) -> dict:
        return self._on_ac_handle(flat, lambda h: h.run_inject(freqs, vph, node_p, node_n, amp, want_currents))

    def run_ac_noise(self, flat: abi.FlatCircuit, freqs, node_p: int, node_n: int, req: abi.SpiceyAcNoiseReq) -> dict:
        """AcHandle.run_noise on a handle of its own: the injected sweep's results never leave the device."""
        return self._on_ac_handle(flat, lambda h: h.run_noise(freqs, node_p, node_n, req))

    def run_ac_sens(self, flat: abi.FlatCircuit, freqs, vph, node_p: int, node_n: int, req: abi.SpiceyAcSensReq, tol, full: bool = False) -> dict:
        """AcHandle.run_sens on a handle of its own: neither sweep's results leave the device."""
        return self._on_ac_handle(flat, lambda h: h.run_sens(freqs, vph, node_p, node_n, req, tol, full))

    def run_ac_mc(self, flat: abi.FlatCircuit, freqs, vph, req: abi.SpiceyAcMcReq, tol, icdf, lo=None, hi=None, probs=()) -> dict:
        """AcHandle.run_mc on a handle of its own: the samples' values and their sweep never leave the device."""
        return self._on_ac_handle(flat, lambda h: h.run_mc(freqs, vph, req, tol, icdf, lo, hi, probs))


class HipBackend(_AcCalls):
    """Backend interface used by spicey_amd.simulate: one handle per call (the reference API is stateless)."""

    def __init__(self, device: int = 0, threads: int = 0, inst_per_wg: int = 0, force_global: bool = False, interpreter: int = 0,
                 geometry: int = 0, wgs_per_inst: int = 0, no_reuse: bool = False, front_cut: int = 0, stage_fronts: bool = False, no_pcr: bool = False, no_rows: bool = False,
                 group_retry: bool = False, group_timeout_ms: int = 0, diagnostics: int = 0):
        self.kw = dict(device=device, threads=threads, inst_per_wg=inst_per_wg, force_global=force_global, interpreter=interpreter,
                       geometry=geometry, wgs_per_inst=wgs_per_inst, no_reuse=no_reuse, front_cut=front_cut, stage_fronts=stage_fronts, no_pcr=no_pcr, no_rows=no_rows,
                       group_retry=group_retry, group_timeout_ms=group_timeout_ms, diagnostics=diagnostics)
        self.info: Optional[dict] = None
        self.group_retries = 0      # summed over this backend's runs (group mode; 0 when healthy)
        self.group_stale_polls = 0
        self.ac_launches: list = []  # instances of every AC handle this backend opened (one handle = one launch)

    def _on_handle(self, flat: abi.FlatCircuit, call) -> dict:
        """call(handle) on a handle of its own: its info and its group-mode counters recorded, closed afterwards."""
        h = Handle(flat, **self.kw)
        try:
            self.info = h.info()
            res = call(h)
            res["group_retries"], res["group_stale_polls"] = h.group_retries(), h.group_stale_polls()
            self.group_retries += res["group_retries"]
            self.group_stale_polls += res["group_stale_polls"]
            return res
        finally:
            h.close()

    def run(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, want_currents: bool = True,
            want_iters: bool = True) -> dict:
        return self._on_handle(flat, lambda h: h.run(steps, dt, src, want_currents, want_iters))

    def _reduced(self, method: str, flat: abi.FlatCircuit, *args) -> dict:
        """Handle.<method>(*args) on a handle of its own: the waveforms never leave the device."""
        return self._on_handle(flat, lambda h: getattr(h, method)(*args))

    def run_measure(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, reqs, want_iters: bool = True) -> dict:
        return self._reduced("run_measure", flat, steps, dt, src, reqs, want_iters)

    def run_measure_fourier(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, reqs, freqs, want_iters: bool = True) -> dict:
        return self._reduced("run_measure_fourier", flat, steps, dt, src, reqs, freqs, want_iters)

    def run_measure_timing(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, reqs, freqs, treqs, want_iters: bool = True) -> dict:
        return self._reduced("run_measure_timing", flat, steps, dt, src, reqs, freqs, treqs, want_iters)

    def run_measure_spectrum(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, reqs, freqs, treqs, sreqs, want_iters: bool = True) -> dict:
        return self._reduced("run_measure_spectrum", flat, steps, dt, src, reqs, freqs, treqs, sreqs, want_iters)

    def run_measure_power(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, reqs, freqs, treqs, sreqs, preqs,
                          want_iters: bool = True) -> dict:
        return self._reduced("run_measure_power", flat, steps, dt, src, reqs, freqs, treqs, sreqs, preqs, want_iters)

    def run_reduced(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, reqs=(), freqs=(), treqs=(), sreqs=(), preqs=(), vreqs=(), pts=(),
                    want_iters: bool = True) -> dict:
        return self._reduced("run_reduced", flat, steps, dt, src, reqs, freqs, treqs, sreqs, preqs, vreqs, pts, want_iters)

    def run_tran_mc(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, req: abi.SpiceyTranMcReq, tol, icdf, scalars, lo=None, hi=None,
                    probs=(), reqs=(), treqs=(), preqs=(), want_x: bool = False) -> dict:
        """Handle.run_mc on a handle of its own whose instances are the samples (flat: the nominal circuit replicated)."""
        return self._on_handle(flat, lambda h: h.run_mc(steps, dt, src, req, tol, icdf, scalars, lo, hi, probs, reqs, treqs, preqs, want_x=want_x))

    def run_tran_sens(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, req: abi.SpiceyTranSensReq, act, step, tol, scalars, reqs=(), treqs=(),
                      preqs=(), want_x: bool = False) -> dict:
        """Handle.run_sens on a handle of its own whose instances are the variants (flat: the nominal circuit replicated 1 + 2 nA times)."""
        return self._on_handle(flat, lambda h: h.run_sens(steps, dt, src, req, act, step, tol, scalars, reqs, treqs, preqs, want_x=want_x))

    def run_tran_levels(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, req: abi.SpiceyTranSensReq, lvl, tol, scalars, reqs=(), treqs=(),
                        preqs=()) -> dict:
        """Handle.run_levels on a handle of its own whose instances are the level rows (flat: the nominal circuit replicated)."""
        return self._on_handle(flat, lambda h: h.run_levels(steps, dt, src, req, lvl, tol, scalars, reqs, treqs, preqs))

    def run_pss(self, flat: abi.FlatCircuit, m_steps: int, dt: float, src: np.ndarray, req: abi.SpiceyPssReq) -> dict:
        """Handle.run_pss on a handle of its own whose instances are the circuits' nominal and perturbed copies."""
        return self._on_handle(flat, lambda h: h.run_pss(m_steps, dt, src, req))

    def run_fit(self, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, req: abi.SpiceyFitReq, act, step, g_lo, g_hi, g0, goals, scalars, reqs=(),
                treqs=(), preqs=()) -> dict:
        """Handle.run_fit on a handle of its own whose instances are the circuits' nominal and perturbed copies."""
        return self._on_handle(flat, lambda h: h.run_fit(steps, dt, src, req, act, step, g_lo, g_hi, g0, goals, scalars, reqs, treqs, preqs))


class HipAcExactBackend(_AcCalls):
    """run_ac through the reference-order AC engine (AcHandle(interpreter=3)): the reference's numbers and errors bit for
    bit.  Used by simulateAC(ckt, exact_order=True)."""

    exact_order = True  # (simulateAC leaves the inductors' "Complex divide by ~0" to the engine, frequency by frequency)
    ac_interpreter = 3

    def __init__(self, device: int = 0, threads: int = 0, force_global: bool = False):
        self.kw = dict(device=device, threads=threads, force_global=force_global)
        self.info: Optional[dict] = None
        self.ac_launches: list = []  # instances of every AC handle this backend opened (one handle = one launch)
