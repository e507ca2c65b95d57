"""ctypes view of include/spicey_hip.h plus ParsedCircuit -> SpiceyDesc flattening.

The flattening is what the TypeScript layer does before its bun:ffi call:
AoS JS objects -> SoA int32/f64 arrays, node ids kept as the reference's ids (0 = ground).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import numpy as np

from .netlist import EPS, ParsedCircuit

ABI_VERSION = 2
OK, ERR_SINGULAR, ERR_BAD_DESC, ERR_HIP, ERR_NO_DEVICE, ERR_COMPLEX_DIV = 0, 1, 2, 3, 4, 5

_I32P = C.POINTER(C.c_int32)
_F64P = C.POINTER(C.c_double)


class SpiceyDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("n_nodes", C.c_int32), ("n_inst", C.c_int32),
        ("nR", C.c_int32), ("nC", C.c_int32), ("nL", C.c_int32), ("nV", C.c_int32), ("nS", C.c_int32), ("nD", C.c_int32),
        ("R_n1", _I32P), ("R_n2", _I32P), ("R_val", _F64P),
        ("C_n1", _I32P), ("C_n2", _I32P), ("C_val", _F64P), ("C_vprev", _F64P),
        ("L_n1", _I32P), ("L_n2", _I32P), ("L_val", _F64P), ("L_iprev", _F64P),
        ("V_n1", _I32P), ("V_n2", _I32P),
        ("S_n1", _I32P), ("S_n2", _I32P), ("S_cp", _I32P), ("S_cn", _I32P),
        ("S_ron", _F64P), ("S_roff", _F64P), ("S_von", _F64P), ("S_voff", _F64P), ("S_ison", _I32P),
        ("D_np", _I32P), ("D_nm", _I32P), ("D_is", _F64P), ("D_n", _F64P), ("D_vdprev", _F64P),
        ("n_out", C.c_int32), ("out_nodes", _I32P),
    ]


class SpiceyOptions(C.Structure):
    _fields_ = [("device", C.c_int32), ("threads", C.c_int32), ("inst_per_wg", C.c_int32),
                ("want_currents", C.c_int32), ("force_global", C.c_int32), ("profile", C.c_int32), ("interpreter", C.c_int32), ("geometry", C.c_int32), ("debug", C.c_int32), ("wgs_per_inst", C.c_int32), ("front_cut", C.c_int32),
                ("group_retry", C.c_int32), ("group_timeout_ms", C.c_int32), ("diagnostics", C.c_int32)]


class SpiceyInfo(C.Structure):
    _fields_ = [("n_var", C.c_int32), ("nnz_a", C.c_int32), ("nnz_lu", C.c_int32), ("n_levels", C.c_int32),
                ("threads", C.c_int32), ("inst_per_wg", C.c_int32), ("lds_bytes", C.c_int32), ("n_cur", C.c_int32),
                ("n_out", C.c_int32), ("n_workgroups", C.c_int32), ("interpreter", C.c_int32), ("geometry", C.c_int32),
                ("tail_levels", C.c_int32), ("wgs_per_inst", C.c_int32), ("resident_slots", C.c_int32),
                ("resident_tasks", C.c_int64), ("streamed_tasks", C.c_int64), ("program_bytes", C.c_int64),
                ("algorithmic_bytes_solve", C.c_int64), ("factor_reuse", C.c_int32), ("n_fronts", C.c_int32),
                ("front_cut", C.c_int32), ("max_front", C.c_int32), ("front_ws_bytes", C.c_int64),
                ("pcr_rows", C.c_int32), ("pcr_level", C.c_int32), ("hybrid_entries", C.c_int32), ("operand_addr", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class SpiceyMeasReq(C.Structure):
    _fields_ = [("kind", C.c_int32), ("signal", C.c_int32), ("col", C.c_int32), ("col_ref", C.c_int32),
                ("step_from", C.c_int64), ("step_to", C.c_int64), ("level", C.c_double), ("dir", C.c_int32), ("reserved", C.c_int32)]


# the same record as a numpy dtype: a request list is one array of these (spicey_amd/measure.py builds them)
MEAS_REQ_DTYPE = np.dtype([("kind", "<i4"), ("signal", "<i4"), ("col", "<i4"), ("col_ref", "<i4"), ("step_from", "<i8"), ("step_to", "<i8"),
                           ("level", "<f8"), ("dir", "<i4"), ("reserved", "<i4")])
assert MEAS_REQ_DTYPE.itemsize == C.sizeof(SpiceyMeasReq) == 48
MEAS_STATS, MEAS_CROSS = 0, 1


class SpiceyFourReq(C.Structure):
    _fields_ = [("signal", C.c_int32), ("col", C.c_int32), ("col_ref", C.c_int32), ("n_harm", C.c_int32),
                ("step_from", C.c_int64), ("step_to", C.c_int64), ("f0", C.c_double)]


# a harmonics request list (spicey_fourier_device) is one array of these
FOUR_REQ_DTYPE = np.dtype([("signal", "<i4"), ("col", "<i4"), ("col_ref", "<i4"), ("n_harm", "<i4"), ("step_from", "<i8"), ("step_to", "<i8"),
                           ("f0", "<f8")])
assert FOUR_REQ_DTYPE.itemsize == C.sizeof(SpiceyFourReq) == 40
FOUR_MAX_HARM = 16


class SpiceyTimingEdge(C.Structure):
    _fields_ = [("signal", C.c_int32), ("col", C.c_int32), ("col_ref", C.c_int32), ("dir", C.c_int32), ("n", C.c_int32), ("level_kind", C.c_int32),
                ("base_from", C.c_int64), ("base_to", C.c_int64), ("level", C.c_double)]


class SpiceyTimingReq(C.Structure):
    _fields_ = [("step_from", C.c_int64), ("step_to", C.c_int64), ("has_trig", C.c_int32), ("targ_from_trig", C.c_int32),
                ("trig", SpiceyTimingEdge), ("targ", SpiceyTimingEdge)]


# an edge-timing request list (spicey_timing_device) is one array of these; trig / targ are nested edge records
TIMING_EDGE_DTYPE = np.dtype([("signal", "<i4"), ("col", "<i4"), ("col_ref", "<i4"), ("dir", "<i4"), ("n", "<i4"), ("level_kind", "<i4"),
                              ("base_from", "<i8"), ("base_to", "<i8"), ("level", "<f8")])
TIMING_REQ_DTYPE = np.dtype([("step_from", "<i8"), ("step_to", "<i8"), ("has_trig", "<i4"), ("targ_from_trig", "<i4"),
                             ("trig", TIMING_EDGE_DTYPE), ("targ", TIMING_EDGE_DTYPE)])
assert TIMING_EDGE_DTYPE.itemsize == C.sizeof(SpiceyTimingEdge) == 48 and TIMING_REQ_DTYPE.itemsize == C.sizeof(SpiceyTimingReq) == 120
TIMING_ABS, TIMING_MINMAX, TIMING_ENDS = 0, 1, 2


class SpiceySpecReq(C.Structure):
    _fields_ = [("signal", C.c_int32), ("col", C.c_int32), ("col_ref", C.c_int32), ("kind", C.c_int32), ("step_from", C.c_int64),
                ("log2n", C.c_int32), ("window", C.c_int32), ("bin_from", C.c_int32), ("bin_to", C.c_int32)]


# a spectrum request list (spicey_spectrum_device) is one array of these
SPEC_REQ_DTYPE = np.dtype([("signal", "<i4"), ("col", "<i4"), ("col_ref", "<i4"), ("kind", "<i4"), ("step_from", "<i8"),
                           ("log2n", "<i4"), ("window", "<i4"), ("bin_from", "<i4"), ("bin_to", "<i4")])
assert SPEC_REQ_DTYPE.itemsize == C.sizeof(SpiceySpecReq) == 40
SPEC_BINS, SPEC_DOMINANT = 0, 1
SPEC_RECT, SPEC_HANN = 0, 1
SPEC_MIN_LOG2N, SPEC_MAX_LOG2N = 3, 13
SPEC_DOM_DOUBLES = 8


def spec_row_doubles(reqs) -> int:
    """Doubles of a result row that holds every request of a spectrum list: 2 per bin of the widest band, 8 for a dominant."""
    r = np.ascontiguousarray(reqs, dtype=SPEC_REQ_DTYPE).reshape(-1)
    if not len(r):
        return 1
    return int(np.where(r["kind"] == SPEC_BINS, 2 * (r["bin_to"].astype(np.int64) - r["bin_from"] + 1), SPEC_DOM_DOUBLES).max())


class SpiceyPowerReq(C.Structure):
    _fields_ = [("a_signal", C.c_int32), ("a_col", C.c_int32), ("a_col_ref", C.c_int32), ("b_signal", C.c_int32), ("b_col", C.c_int32),
                ("b_col_ref", C.c_int32), ("neg", C.c_int32), ("reserved", C.c_int32), ("step_from", C.c_int64), ("step_to", C.c_int64)]


# a list of products of two signals (spicey_power_device) is one array of these
POWER_REQ_DTYPE = np.dtype([("a_signal", "<i4"), ("a_col", "<i4"), ("a_col_ref", "<i4"), ("b_signal", "<i4"), ("b_col", "<i4"), ("b_col_ref", "<i4"),
                            ("neg", "<i4"), ("reserved", "<i4"), ("step_from", "<i8"), ("step_to", "<i8")])
assert POWER_REQ_DTYPE.itemsize == C.sizeof(SpiceyPowerReq) == 48
POWER_REQ = POWER_REQ_DTYPE
POWER_ROW = 16


class SpiceyValReq(C.Structure):
    _fields_ = [("kind", C.c_int32), ("signal", C.c_int32), ("col", C.c_int32), ("col_ref", C.c_int32), ("x_signal", C.c_int32), ("x_col", C.c_int32),
                ("x_col_ref", C.c_int32), ("timing_row", C.c_int32), ("step_from", C.c_int64), ("step_to", C.c_int64), ("first", C.c_int64),
                ("count", C.c_int64), ("buckets", C.c_int32), ("reserved", C.c_int32)]


class SpiceyValPoint(C.Structure):
    _fields_ = [("k", C.c_int64), ("f", C.c_double)]


# a list of waveform-value requests (spicey_values_device) is one array of VAL_REQ_DTYPE, its point table one of VAL_POINT_DTYPE
VAL_REQ_DTYPE = np.dtype([("kind", "<i4"), ("signal", "<i4"), ("col", "<i4"), ("col_ref", "<i4"), ("x_signal", "<i4"), ("x_col", "<i4"), ("x_col_ref", "<i4"),
                          ("timing_row", "<i4"), ("step_from", "<i8"), ("step_to", "<i8"), ("first", "<i8"), ("count", "<i8"), ("buckets", "<i4"),
                          ("reserved", "<i4")])
VAL_POINT_DTYPE = np.dtype([("k", "<i8"), ("f", "<f8")])
assert VAL_REQ_DTYPE.itemsize == C.sizeof(SpiceyValReq) == 72 and VAL_POINT_DTYPE.itemsize == C.sizeof(SpiceyValPoint) == 16
VAL_TRACE, VAL_POINTS, VAL_FIND = 0, 1, 2
TRACE_MAX_BUCKETS = 4096
VAL_TRACE_DOUBLES, VAL_POINT_DOUBLES = 6, 4


def val_row_doubles(reqs) -> int:
    """Doubles of a result row that holds every request of a values list: 6 per bucket, 4 per point, 4 for a find."""
    r = np.ascontiguousarray(reqs, dtype=VAL_REQ_DTYPE).reshape(-1)
    if not len(r):
        return 1
    return int(np.where(r["kind"] == VAL_TRACE, VAL_TRACE_DOUBLES * r["buckets"].astype(np.int64),
                        np.where(r["kind"] == VAL_POINTS, VAL_POINT_DOUBLES * r["count"], VAL_POINT_DOUBLES)).max())


class SpiceyReducedLists(C.Structure):
    """The lists of spicey_run_reduced (include/spicey_hip.h); struct_bytes = C.sizeof(SpiceyReducedLists)."""
    _fields_ = [("struct_bytes", C.c_int64),
                ("reqs", C.c_void_p), ("meas", C.c_void_p), ("freqs", C.c_void_p), ("four", C.c_void_p), ("treqs", C.c_void_p), ("timing", C.c_void_p),
                ("sreqs", C.c_void_p), ("spec", C.c_void_p), ("preqs", C.c_void_p), ("power", C.c_void_p),
                ("n_req", C.c_int32), ("n_four", C.c_int32), ("four_stride", C.c_int32), ("n_timing", C.c_int32), ("n_spec", C.c_int32),
                ("spec_stride", C.c_int32), ("n_power", C.c_int32), ("n_values", C.c_int32),
                ("vreqs", C.c_void_p), ("values", C.c_void_p), ("pts", C.c_void_p), ("n_pts", C.c_int64), ("values_stride", C.c_int32),
                ("reserved", C.c_int32)]


assert C.sizeof(SpiceyReducedLists) == 160


class SpiceyAcMeasReq(C.Structure):
    _fields_ = [("num_signal", C.c_int32), ("num_col", C.c_int32), ("num_col_ref", C.c_int32),
                ("den_signal", C.c_int32), ("den_col", C.c_int32), ("den_col_ref", C.c_int32), ("what", C.c_int32), ("kind", C.c_int32),
                ("k_from", C.c_int64), ("k_to", C.c_int64), ("level", C.c_double),
                ("dir", C.c_int32), ("which", C.c_int32), ("rel", C.c_int32), ("reserved", C.c_int32)]


# one request of an AC measurement (include/spicey_hip.h, SpiceyAcMeasReq; spicey_amd/ac_measure.py builds them)
AC_MEAS_REQ_DTYPE = np.dtype([("num_signal", "<i4"), ("num_col", "<i4"), ("num_col_ref", "<i4"), ("den_signal", "<i4"), ("den_col", "<i4"),
                              ("den_col_ref", "<i4"), ("what", "<i4"), ("kind", "<i4"), ("k_from", "<i8"), ("k_to", "<i8"), ("level", "<f8"),
                              ("dir", "<i4"), ("which", "<i4"), ("rel", "<i4"), ("reserved", "<i4")])
assert AC_MEAS_REQ_DTYPE.itemsize == C.sizeof(SpiceyAcMeasReq) == 72
AC_MEAS_EXTREMA, AC_MEAS_CROSS = 0, 1
AC_WHAT_MAG2, AC_WHAT_RE, AC_WHAT_IM = 0, 1, 2


class SpiceyAcInject(C.Structure):
    """The injected current of spicey_ac_run_inject / spicey_ac_run_noise; struct_bytes = C.sizeof(SpiceyAcInject)."""
    _fields_ = [("struct_bytes", C.c_int64), ("node_p", C.c_int32), ("node_n", C.c_int32), ("re", C.c_double), ("im", C.c_double)]


class SpiceyAcNoiseReq(C.Structure):
    """The request of the noise pass (include/spicey_hip.h); struct_bytes = C.sizeof(SpiceyAcNoiseReq)."""
    _fields_ = [("struct_bytes", C.c_int64), ("out_p", C.c_int32), ("out_n", C.c_int32), ("in_col", C.c_int32), ("reserved", C.c_int32),
                ("k_from", C.c_int64), ("k_to", C.c_int64), ("kt4", C.c_double)]


assert C.sizeof(SpiceyAcInject) == 32 and C.sizeof(SpiceyAcNoiseReq) == 48
NOISE_SPEC = 4  # doubles of a row of d_spec: onoise, gain2, zout_re, zout_im


def ac_inject(node_p: int, node_n: int, amp: complex = 1.0) -> SpiceyAcInject:
    return SpiceyAcInject(C.sizeof(SpiceyAcInject), int(node_p), int(node_n), float(complex(amp).real), float(complex(amp).imag))


def ac_noise_req(out_p: int, out_n: int, in_col: int, kt4: float, k_from: int = 0, k_to: int = -1) -> SpiceyAcNoiseReq:
    return SpiceyAcNoiseReq(C.sizeof(SpiceyAcNoiseReq), int(out_p), int(out_n), int(in_col), 0, int(k_from), int(k_to), float(kt4))


class SpiceyAcSensReq(C.Structure):
    """The request of the sensitivity pass (include/spicey_hip.h); struct_bytes = C.sizeof(SpiceyAcSensReq)."""
    _fields_ = [("struct_bytes", C.c_int64), ("out_p", C.c_int32), ("out_n", C.c_int32), ("nR", C.c_int32), ("nC", C.c_int32), ("nL", C.c_int32),
                ("reserved", C.c_int32), ("k_from", C.c_int64), ("k_to", C.c_int64)]


assert C.sizeof(SpiceyAcSensReq) == 48
SENS_SPEC = 6  # doubles of a row of d_spec: h_re, h_im, wc_mag, var_mag, wc_ph, var_ph
SENS_PEAK = 4  # doubles of a row of d_peak: m at its peak, its frequency index, phi at its peak, its frequency index


def ac_sens_req(out_p: int, out_n: int, nR: int, nC: int, nL: int, k_from: int = 0, k_to: int = -1) -> SpiceyAcSensReq:
    return SpiceyAcSensReq(C.sizeof(SpiceyAcSensReq), int(out_p), int(out_n), int(nR), int(nC), int(nL), 0, int(k_from), int(k_to))


class SpiceyAcMcReq(C.Structure):
    """The request of the Monte Carlo pass (include/spicey_hip.h); struct_bytes = C.sizeof(SpiceyAcMcReq)."""
    _fields_ = [("struct_bytes", C.c_int64), ("out_p", C.c_int32), ("out_n", C.c_int32), ("log2K", C.c_int32), ("keep_first", C.c_int32),
                ("seed", C.c_uint64), ("reserved", C.c_int64)]


assert C.sizeof(SpiceyAcMcReq) == 40
MC_FREQ_HEAD = 4    # doubles of a row of d_freq before the order statistics: n_valid, violating samples, sum q, sum q q
MC_MAX_INST = 16384  # samples one workgroup sorts in LDS
MC_MAX_LOG2K = 12


def ac_mc_req(out_p: int, out_n: int, log2K: int, keep_first: bool = True, seed: int = 0) -> SpiceyAcMcReq:
    return SpiceyAcMcReq(C.sizeof(SpiceyAcMcReq), int(out_p), int(out_n), int(log2K), int(bool(keep_first)), int(seed) & 0xFFFFFFFFFFFFFFFF, 0)


class SpiceyTranMcReq(C.Structure):
    """The request of a Monte Carlo of transient runs (include/spicey_hip.h); struct_bytes = C.sizeof(SpiceyTranMcReq)."""
    _fields_ = [("struct_bytes", C.c_int64), ("log2K", C.c_int32), ("keep_first", C.c_int32), ("seed", C.c_uint64), ("reserved", C.c_int64)]


class SpiceyMcRows(C.Structure):
    """The device rows of one pass for spicey_tran_mc_reduce_device: [n_inst][n_rows][stride]."""
    _fields_ = [("d_rows", C.c_void_p), ("n_rows", C.c_int32), ("stride", C.c_int32)]


# one instruction of a scalar's program and the program (include/spicey_hip.h, SpiceyMcIns / SpiceyMcScalar; spicey_amd/tran_mc.py builds them)
MC_INS_DTYPE = np.dtype([("op", "<i4"), ("pass", "<i4"), ("row", "<i4"), ("field", "<i4"), ("c", "<f8")])
MC_SCALAR_INS, MC_SCALAR_STACK = 48, 4
MC_SCALAR_DTYPE = np.dtype([("n_ins", "<i4"), ("reserved", "<i4"), ("ins", MC_INS_DTYPE, (MC_SCALAR_INS,))])
assert C.sizeof(SpiceyTranMcReq) == 32 and C.sizeof(SpiceyMcRows) == 16 and MC_INS_DTYPE.itemsize == 24 and MC_SCALAR_DTYPE.itemsize == 1160
MCOP_FIELD, MCOP_CONST, MCOP_ADD, MCOP_SUB, MCOP_MUL, MCOP_DIV, MCOP_GUARD = 1, 2, 3, 4, 5, 6, 7
MC_PASS_MEASURE, MC_PASS_TIMING, MC_PASS_POWER = 0, 1, 2
MC_PASS_STRIDE = (8, 8, POWER_ROW)
TRAN_MC_STAT_HEAD = 8  # doubles of a row of d_stat before the order statistics: n_valid, n_num, n_viol, sum x, sum x x, s_min, s_max, 0


def tran_mc_req(log2K: int, keep_first: bool = True, seed: int = 0) -> SpiceyTranMcReq:
    return SpiceyTranMcReq(C.sizeof(SpiceyTranMcReq), int(log2K), int(bool(keep_first)), int(seed) & 0xFFFFFFFFFFFFFFFF, 0)


class SpiceyTranSensReq(C.Structure):
    """The request of a sensitivity or levels run of transient measurements (include/spicey_hip.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("mode", C.c_int32), ("nA", C.c_int32), ("reserved", C.c_int64 * 2)]


assert C.sizeof(SpiceyTranSensReq) == 32
TS_ONE_AT_A_TIME, TS_LEVELS = 0, 1
TRAN_SENS_BOUND_ROW = 8  # doubles of a row of d_bound: x0, wc, rss2, n_num, a_max, contrib_max, n_interior, 0


def tran_sens_req(mode: int, nA: int = 0) -> SpiceyTranSensReq:
    return SpiceyTranSensReq(C.sizeof(SpiceyTranSensReq), int(mode), int(nA))


class SpiceyPssReq(C.Structure):
    """The request of a periodic-steady-state design, update or run (include/spicey_hip.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("n_ckt", C.c_int32), ("method", C.c_int32), ("max_iter", C.c_int32), ("pad", C.c_int32),
                ("damping", C.c_double), ("reltol", C.c_double), ("vabstol", C.c_double), ("iabstol", C.c_double), ("rel_step", C.c_double),
                ("v_scale", C.c_double), ("i_scale", C.c_double), ("reserved", C.c_int64)]


assert C.sizeof(SpiceyPssReq) == 88
PSS_NEWTON, PSS_SETTLE = 0, 1
PSS_METHODS = {"newton": PSS_NEWTON, "settle": PSS_SETTLE}
PSS_MAX_NX = 128  # states of one circuit the Newton update takes
PSS_ROW = 8  # doubles of a row: res, step, n_switch_mismatch, status, a_res, min |pivot|, n_pert_switch_diff, converged
PSS_ROW_KEYS = ("res", "step", "n_switch_mismatch", "status", "a_res", "min_pivot", "n_pert_switch_diff", "converged")
# a circuit's status: converged, max_iter reached (a row: moved), the nominal's run singular, singular Jacobian, a value that is
# not finite or a singular perturbed instance, stopped by another circuit's failure
PSS_CONVERGED, PSS_MAX_ITER, PSS_NOMINAL_SINGULAR, PSS_SINGULAR_JACOBIAN, PSS_NOT_FINITE, PSS_STOPPED = 0, 1, 2, 3, 4, 5


def pss_req(n_ckt: int, method: int = PSS_NEWTON, max_iter: int = 20, damping: float = 1.0, reltol: float = 1e-6, vabstol: float = 1e-9,
            iabstol: float = 1e-12, rel_step: float = 1e-6, v_scale: float = 1.0, i_scale: float = 1e-3) -> SpiceyPssReq:
    return SpiceyPssReq(C.sizeof(SpiceyPssReq), int(n_ckt), int(method), int(max_iter), 0, float(damping), float(reltol), float(vabstol), float(iabstol),
                        float(rel_step), float(v_scale), float(i_scale), 0)


def pss_width(method: int, nX: int) -> int:
    """Instances per circuit: the nominal and, with Newton, one per perturbed state entry."""
    return 1 if method == PSS_SETTLE else 1 + nX


class SpiceyFitReq(C.Structure):
    """The request of an element-sizing design, update or run (include/spicey_hip.h)."""
    _fields_ = [("struct_bytes", C.c_int64), ("n_ckt", C.c_int32), ("nA", C.c_int32), ("max_iter", C.c_int32), ("pad", C.c_int32),
                ("lambda0", C.c_double), ("lam_up", C.c_double), ("lam_down", C.c_double), ("lam_max", C.c_double), ("max_step", C.c_double),
                ("x_tol", C.c_double), ("f_tol", C.c_double), ("pivot_min", C.c_double), ("reserved", C.c_int64)]


assert C.sizeof(SpiceyFitReq) == 96
# a goal on one scalar (include/spicey_hip.h, SpiceyFitGoal)
FIT_GOAL_DTYPE = np.dtype([("kind", "<i4"), ("pad", "<i4"), ("lo", "<f8"), ("hi", "<f8"), ("weight", "<f8")])
assert FIT_GOAL_DTYPE.itemsize == 32
FIT_EQ, FIT_AT_MOST, FIT_AT_LEAST, FIT_BETWEEN = 0, 1, 2, 3
FIT_MAX_NA = 128  # active elements of one circuit the update takes
FIT_ROW = 8  # doubles of a row: F, F_good, lambda, accepted, status, max |d|, n_frozen, n_clamped
FIT_ROW_KEYS = ("F", "F_good", "lambda", "accepted", "status", "max_step", "n_frozen", "n_clamped")
# a circuit's status: converged, max_iter reached (a row: moved), the first nominal not evaluable, singular system, a value that is
# not finite, stalled (lambda passed lam_max)
FIT_CONVERGED, FIT_MAX_ITER, FIT_NOT_EVALUABLE, FIT_SINGULAR, FIT_NOT_FINITE, FIT_STALLED = 0, 1, 2, 3, 4, 5


def fit_req(n_ckt: int, nA: int, max_iter: int = 30, lambda0: float = 1e-3, lam_up: float = 10.0, lam_down: float = 0.1, lam_max: float = 1e8,
            max_step: float = 0.5, x_tol: float = 1e-6, f_tol: float = 1e-12, pivot_min: float = 1e-300) -> SpiceyFitReq:
    return SpiceyFitReq(C.sizeof(SpiceyFitReq), int(n_ckt), int(nA), int(max_iter), 0, float(lambda0), float(lam_up), float(lam_down), float(lam_max),
                        float(max_step), float(x_tol), float(f_tol), float(pivot_min), 0)


def fit_goals(rows) -> np.ndarray:
    """[(kind, lo, hi, weight)] as records of FIT_GOAL_DTYPE."""
    out = np.zeros(len(rows), FIT_GOAL_DTYPE)
    for k, (kind, lo, hi, w) in enumerate(rows):
        out[k] = (int(kind), 0, float(lo), float(hi), float(w))
    return out


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


class FlatCircuit:
    """Owns the numpy arrays a SpiceyDesc points into.

    ``n_inst`` instances share the topology; per-instance value arrays have shape [n_inst, n].
    """

    TOPO = ("R_n1", "R_n2", "C_n1", "C_n2", "L_n1", "L_n2", "V_n1", "V_n2", "S_n1", "S_n2", "S_cp", "S_cn", "D_np", "D_nm")
    VALS = ("R_val", "C_val", "C_vprev", "L_val", "L_iprev", "S_ron", "S_roff", "S_von", "S_voff", "D_is", "D_n", "D_vdprev")
    _KIND = {"R": "nR", "C": "nC", "L": "nL", "V": "nV", "S": "nS", "D": "nD"}

    def __init__(self, n_nodes: int, n_inst: int = 1, **arrays) -> None:
        self.n_nodes = int(n_nodes)
        self.n_inst = int(n_inst)
        self.out_nodes: Optional[np.ndarray] = None
        for k in self.TOPO:
            setattr(self, k, _i32(arrays.get(k, [])))
        self.nR, self.nC, self.nL = len(self.R_n1), len(self.C_n1), len(self.L_n1)
        self.nV, self.nS, self.nD = len(self.V_n1), len(self.S_n1), len(self.D_np)
        for k in self.VALS:
            n = getattr(self, self._KIND[k[0]])
            a = arrays.get(k)
            a = np.zeros((self.n_inst, n)) if a is None else _f64(a).reshape(self.n_inst, n)
            setattr(self, k, a)
        ison = arrays.get("S_ison")
        self.S_ison = np.zeros((self.n_inst, self.nS), np.int32) if ison is None else _i32(ison).reshape(self.n_inst, self.nS)
        if arrays.get("out_nodes") is not None:
            self.out_nodes = _i32(arrays["out_nodes"])

    @property
    def n_var(self) -> int:
        return self.n_nodes + self.nV

    @property
    def n_cur(self) -> int:
        return self.nR + self.nC + self.nL + self.nV + self.nS + self.nD

    @property
    def n_out(self) -> int:
        return len(self.out_nodes) if self.out_nodes is not None and len(self.out_nodes) else self.n_nodes

    def desc(self) -> SpiceyDesc:
        d = SpiceyDesc()
        d.abi_version = ABI_VERSION
        d.n_nodes, d.n_inst = self.n_nodes, self.n_inst
        d.nR, d.nC, d.nL, d.nV, d.nS, d.nD = self.nR, self.nC, self.nL, self.nV, self.nS, self.nD
        for k in self.TOPO + ("S_ison",):
            setattr(d, k, getattr(self, k).ctypes.data_as(_I32P))
        for k in self.VALS:
            setattr(d, k, getattr(self, k).ctypes.data_as(_F64P))
        if self.out_nodes is not None and len(self.out_nodes):
            d.n_out = len(self.out_nodes)
            d.out_nodes = self.out_nodes.ctypes.data_as(_I32P)
        else:
            d.n_out = 0
            d.out_nodes = None
        d._keepalive = self  # the arrays must outlive the struct
        return d

    def replicate(self, n_inst: int) -> "FlatCircuit":
        """Same topology, values of instance 0 copied to n_inst instances."""
        kw = {k: getattr(self, k) for k in self.TOPO}
        for k in self.VALS + ("S_ison",):
            kw[k] = np.repeat(getattr(self, k)[:1], n_inst, axis=0)
        kw["out_nodes"] = self.out_nodes
        return FlatCircuit(self.n_nodes, n_inst, **kw)


def flatten(ckt: ParsedCircuit, probe_filter: bool = False) -> FlatCircuit:
    """ParsedCircuit (one instance) -> FlatCircuit; state fields are the circuit's CURRENT state,
    so a second simulateTRAN continues where the first stopped."""
    out_nodes = None
    if probe_filter and len(ckt.probes["tran"]) > 0:
        upper = [p.upper() for p in ckt.probes["tran"]]
        out_nodes = [i for i in range(1, ckt.nodes.count()) if ckt.nodes.rev[i].upper() in upper]
    S = [s for s in ckt.S if s.model is not None]
    D = [d for d in ckt.D if d.model is not None]
    return FlatCircuit(
        ckt.nodes.count() - 1, 1,
        R_n1=[e.n1 for e in ckt.R], R_n2=[e.n2 for e in ckt.R], R_val=[e.R for e in ckt.R],
        C_n1=[e.n1 for e in ckt.C], C_n2=[e.n2 for e in ckt.C], C_val=[e.C for e in ckt.C], C_vprev=[e.vPrev for e in ckt.C],
        L_n1=[e.n1 for e in ckt.L], L_n2=[e.n2 for e in ckt.L], L_val=[e.L for e in ckt.L], L_iprev=[e.iPrev for e in ckt.L],
        V_n1=[e.n1 for e in ckt.V], V_n2=[e.n2 for e in ckt.V],
        S_n1=[e.n1 for e in S], S_n2=[e.n2 for e in S], S_cp=[e.ncPos for e in S], S_cn=[e.ncNeg for e in S],
        S_ron=[e.model.Ron for e in S], S_roff=[e.model.Roff for e in S],
        S_von=[e.model.Von for e in S], S_voff=[e.model.Voff for e in S], S_ison=[1 if e.isOn else 0 for e in S],
        D_np=[e.nPlus for e in D], D_nm=[e.nMinus for e in D], D_is=[e.model.Is for e in D], D_n=[e.model.N for e in D],
        D_vdprev=[e.vdPrev for e in D],
        out_nodes=out_nodes,
    )


def stack_instances(flats: Sequence[FlatCircuit]) -> FlatCircuit:
    """Batch circuits that share one topology (parameter sweeps, BASELINE config 4)."""
    f0 = flats[0]
    for f in flats[1:]:
        for k in FlatCircuit.TOPO:
            if not np.array_equal(getattr(f, k), getattr(f0, k)) or f.n_nodes != f0.n_nodes:
                raise ValueError("instances of one batch must share the topology (" + k + " differs)")
    kw = {k: getattr(f0, k) for k in FlatCircuit.TOPO}
    for k in FlatCircuit.VALS + ("S_ison",):
        kw[k] = np.concatenate([getattr(f, k) for f in flats], axis=0)
    kw["out_nodes"] = f0.out_nodes
    return FlatCircuit(f0.n_nodes, sum(f.n_inst for f in flats), **kw)


def computeEffectiveTimeStep(dt_requested: float, tstop: float):
    """simulateTRAN.ts:14-19, same double operations in the same order."""
    dt_eff = dt_requested if dt_requested > EPS else max(tstop / 1000, EPS)
    steps = max(1, math.ceil(tstop / max(dt_eff, EPS)))
    dt = tstop / steps if steps > 0 else tstop
    return dt, steps


def source_table(ckt: ParsedCircuit, dt: float, steps: int) -> np.ndarray:
    """Pre-evaluate `vs.waveform ? vs.waveform(t) : vs.dc || 0` (simulateTRAN.ts:67) at
    t = step*dt (:147) — closures cannot cross the FFI."""
    nv = len(ckt.V)
    tab = np.zeros((steps + 1, nv), dtype=np.float64)
    for k, vs in enumerate(ckt.V):
        if vs.waveform is not None:
            wf = vs.waveform
            tab[:, k] = [wf(step * dt) for step in range(steps + 1)]
        else:
            dc = vs.dc
            tab[:, k] = 0.0 if (dc == 0 or dc != dc) else dc
    return tab


def source_tables(ckts: Sequence[ParsedCircuit], dt: float, steps: int) -> np.ndarray:
    """One source table per circuit, stacked: [len(ckts)][steps+1][nV] — the per-instance layout of spicey_run_src.  The
    circuits must have the same number of voltage sources."""
    tabs = [source_table(c, dt, steps) for c in ckts]
    if len({t.shape for t in tabs}) > 1:
        raise ValueError("source_tables: the circuits differ in their number of voltage sources")
    return np.stack(tabs) if tabs else np.zeros((0, steps + 1, 0))
