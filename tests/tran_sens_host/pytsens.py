"""ctypes view of the CPU harness of the sensitivities and corners of transient measurements (tests/tran_sens_host/harness.cpp):
the design and the reduction of tran_sens_exec.h, plus the inputs the host and GPU tests share."""
import ctypes as C
import os

import numpy as np

import harness_build
from noise_host.pynoise import Refused, bits_equal  # noqa: F401  (the tests' names for them)
from spicey_amd import abi
from spicey_amd import tran_mc as tm
from spicey_amd import tran_sens as ts
from tran_mc_host import pytmc

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SENTINEL = -7.25
SENTINEL_I = -99
NA = (1, 2, 63, 64, 65, 130)
NS = (1, 5)
CASES = ("plain", "all_nan", "invalid_perturbed", "equal_pair", "ties", "interior")
THREADS = (64, 256)


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_tran_sens_host.so")
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.spicey_ts_host_workspace_bytes.restype = i64
        L.spicey_ts_host_workspace_bytes.argtypes = [i32, i32, i32, i32]
        L.spicey_ts_host_design.restype = i32
        L.spicey_ts_host_design.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, C.c_char_p, i32]
        L.spicey_ts_host_reduce.restype = i32
        L.spicey_ts_host_reduce.argtypes = [i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, i64, i32, C.c_char_p, i32]
        assert L.spicey_ts_host_req_bytes() == C.sizeof(abi.SpiceyTranSensReq)
        _LIB = L
    return _LIB


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _arr(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def design(R, Cv, Lv, req, act=None, step=None, lvl=None, tol=None, n_inst=None, nR=None, have_work=True, work_bytes=-1):
    """(R', C', L') of the harness — ohms, farads, henries — for nominal R / Cv / Lv [ni][n<kind>] and a request
    abi.tran_sens_req(...).  A refusal raises Refused with the judge's text, after checking that the results kept their sentinel."""
    ni0 = np.asarray(R).shape[0]
    R, Cv, Lv = (np.ascontiguousarray(a, dtype=np.float64).reshape(ni0, -1) for a in (R, Cv, Lv))
    act, step, lvl, tol = _arr(act, np.int32), _arr(step, np.float64), _arr(lvl, np.int8), _arr(tol, np.float64)
    oR, oC, oL = (np.full(a.shape, SENTINEL) for a in (R, Cv, Lv))
    err = C.create_string_buffer(256)
    rc = lib().spicey_ts_host_design(ni0 if n_inst is None else n_inst, R.shape[1] if nR is None else nR, Cv.shape[1], Lv.shape[1], _ptr(R), _ptr(Cv), _ptr(Lv),
                                     C.addressof(req) if req is not None else None, _ptr(act), _ptr(step), _ptr(lvl), _ptr(tol), _ptr(oR), _ptr(oC), _ptr(oL),
                                     int(have_work), work_bytes, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and (oR == SENTINEL).all() and (oC == SENTINEL).all() and (oL == SENTINEL).all()
        raise Refused(err.value.decode())
    return oR, oC, oL


def reduce(rows, scalars, valid, step, tol_act, n_inst=None, nA=None, have_out=True, work_bytes=-1, threads=0):
    """(x [ni][ns], sens [ns][nA][2], sign [ns][nA] int8, bound [ns][8]) of the harness.  threads: the emulated workgroup.  A
    refusal raises Refused, after checking that the results kept their sentinel."""
    ni0 = next(np.asarray(r).shape[0] for r in rows if r is not None)
    sc = np.ascontiguousarray(scalars, dtype=abi.MC_SCALAR_DTYPE).reshape(-1)
    ns = len(sc)
    arr, keep = pytmc.rows_struct(rows)
    valid, step, tol_act = _arr(valid, np.uint8), _arr(step, np.float64), _arr(tol_act, np.float64)
    na = max((ni0 - 1) // 2, 1)
    x = np.full((ni0, max(ns, 1)), SENTINEL)
    sens = np.full((max(ns, 1), na, 2), SENTINEL)
    sign = np.full((max(ns, 1), na), SENTINEL_I, np.int8)
    bound = np.full((max(ns, 1), abi.TRAN_SENS_BOUND_ROW), SENTINEL)
    err = C.create_string_buffer(256)
    with np.errstate(all="ignore"):
        rc = lib().spicey_ts_host_reduce(ni0 if n_inst is None else n_inst, C.addressof(arr), _ptr(sc), ns, None if valid is None else valid.ctypes.data, _ptr(step),
                                         _ptr(tol_act), (len(step) if step is not None else 0) if nA is None else nA, x.ctypes.data, sens.ctypes.data, sign.ctypes.data,
                                         bound.ctypes.data, int(have_out), work_bytes, threads, err, 256)
    del keep
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and (x == SENTINEL).all() and (sens == SENTINEL).all() and (sign == SENTINEL_I).all() and (bound == SENTINEL).all()
        raise Refused(err.value.decode())
    return x, sens, sign, bound


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
def design_inputs(nA, shape, seed):
    """(R, Cv, Lv [1 + 2 nA][n<kind>], act [nA] with gaps, step [nA], lvl [ni][nE], tol [nE]) of a seeded design; shape = (nR, nC, nL)
    with nR + nC + nL >= nA."""
    rng = np.random.default_rng(seed)
    nR, nC, nL = shape
    nE, ni = nR + nC + nL, 1 + 2 * nA
    R = 10.0 ** rng.uniform(0, 6, (ni, nR))
    Cv = 10.0 ** rng.uniform(-12, -6, (ni, nC))
    Lv = 10.0 ** rng.uniform(-9, -3, (ni, nL))
    act = np.sort(rng.choice(nE, nA, replace=False)).astype(np.int32)
    step = 10.0 ** rng.uniform(-6, -1, nA)
    lvl = rng.integers(-1, 2, (ni, nE)).astype(np.int8)
    lvl[0] = 0
    tol = rng.uniform(0.0, 0.3, nE)
    tol[::5] = 0.0
    return R, Cv, Lv, act, step, lvl, tol


def case_inputs(case, nA, ns, seed):
    """(rows, scalars, valid, step, tol_act) of a named reduction case: every scalar j reads measure row j, field 7."""
    rng = np.random.default_rng(seed)
    ni = 1 + 2 * nA
    step = 10.0 ** rng.uniform(-4, -2, nA)
    tol = rng.uniform(0.01, 0.2, nA)
    x0 = rng.normal(0.0, 1.0, ns)
    slope = rng.normal(0.0, 1.0, (nA, ns)) * 10.0 ** rng.uniform(-2, 2, (nA, ns))
    curv = rng.normal(0.0, 1.0, (nA, ns))
    x = np.empty((ni, ns))
    x[0] = x0
    x[1::2] = x0 + slope * step[:, None] + 0.5 * curv * step[:, None] ** 2
    x[2::2] = x0 - slope * step[:, None] + 0.5 * curv * step[:, None] ** 2
    valid = None
    if case == "all_nan":
        x[:, 0] = np.nan
    elif case == "invalid_perturbed":
        valid = np.ones(ni, np.uint8)
        valid[2 + 2 * (nA // 2)] = 0
        if nA > 2:
            valid[1] = 0
    elif case == "equal_pair":
        x[2 + 2 * (nA - 1)] = x[1 + 2 * (nA - 1)]  # d = 0: sign 0
    elif case == "ties":
        # |d| t equal in elements 0 and nA - 1 of scalar 0 and larger than every other: the lowest index wins
        step[:] = 2.0 ** -10
        tol[:] = 0.125
        x[:, 0] = 1.0
        for a in (0, nA - 1):
            x[1 + 2 * a, 0], x[2 + 2 * a, 0] = 1.0 + 1024.0 * step[a], 1.0 - 1024.0 * step[a]
    elif case == "interior":
        # scalar 0, exact in binary: element 0 has |d| = 1/8 < |c| t = 2 * 1/8 (counted), the last element |d| = |c| t (not counted)
        step[:] = 2.0 ** -8
        tol[:] = 0.125
        x[:, 0] = 1.0
        h = 2.0 ** -8
        x[1, 0], x[2, 0] = 1.0 + 0.125 * h + h * h, 1.0 - 0.125 * h + h * h      # d = 1/8, c = 2
        a = nA - 1
        if a > 0:
            x[1 + 2 * a, 0], x[2 + 2 * a, 0] = 1.0 + 0.25 * h + h * h, 1.0 - 0.25 * h + h * h  # d = 1/4, c = 2: equality
    rows = np.zeros((ni, ns, 8))
    rows[:, :, 7] = x
    scalars = tm.make_scalars([[tm.F(0, j, 7)] for j in range(ns)])
    return (rows, None, None), scalars, valid, step, tol


def designed_flat(flat, act=None, step=None, lvl=None, tol=None):
    """A FlatCircuit whose value rows are the numpy design's (ohms, farads, henries): what a sensitivity or levels run's transient reads."""
    from mc_host.pymc import replicate_rows
    out = replicate_rows(flat)
    out.R_val, out.C_val, out.L_val = (np.ascontiguousarray(a) for a in ts.design_values(out.R_val, out.C_val, out.L_val, act, step, lvl, tol))
    return out


def _oracle_run(designed, steps, dt, src):
    from oracle.pyoracle import OracleBackend
    parts = [OracleBackend().run(pytmc.flat_row(designed, k), steps, dt, src) for k in range(designed.n_inst)]
    ist = np.array([p["status"] for p in parts], np.int32)
    bad = [p for p in parts if p["status"] != abi.OK]
    return {"status": bad[0]["status"] if bad else abi.OK, "detail": bad[0]["detail"] if bad else "", "inst_status": ist,
            "out_v": np.concatenate([p["out_v"] for p in parts]), "out_i": np.concatenate([p["out_i"] for p in parts])}


class HostTranSensBackend:
    """run_tran_sens / run_tran_levels of a backend on the CPU: the numpy design, the oracle's transient per variant, the numpy rows
    of the passes, the harness's scalars and reduction."""

    def run_tran_sens(self, flat, steps, dt, src, req, act, step, tol, scalars, reqs=(), treqs=(), preqs=(), want_x=False):
        res = _oracle_run(designed_flat(flat, act, step), steps, dt, src)
        ist = res["inst_status"]
        out = {"status": res["status"], "detail": res["detail"], "inst_status": ist}
        if ist[0] == 0:
            rows = pytmc.reference_rows(res["out_v"], res["out_i"], reqs, treqs, preqs, dt)
            valid = None if (ist == 0).all() else (ist == 0).astype(np.uint8)
            out["x"], out["sens"], out["sign"], out["bound"] = reduce(rows, scalars, valid, step, np.asarray(tol)[np.asarray(act)])
        return out

    def run_tran_levels(self, flat, steps, dt, src, req, lvl, tol, scalars, reqs=(), treqs=(), preqs=()):
        res = _oracle_run(designed_flat(flat, lvl=lvl, tol=tol), steps, dt, src)
        ist = res["inst_status"]
        out = {"status": res["status"], "detail": res["detail"], "inst_status": ist}
        if (ist == 0).any():
            rows = pytmc.reference_rows(res["out_v"], res["out_i"], reqs, treqs, preqs, dt)
            out["x"] = tm.eval_reference_scalars(scalars, rows, None if (ist == 0).all() else (ist == 0).astype(np.uint8))
        return out
