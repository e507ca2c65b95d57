"""ctypes view of the CPU harness of the Monte Carlo of transient runs (tests/tran_mc_host/harness.cpp): the draw, the scalar
programs and the reduction of tran_mc_exec.h, plus the inputs the host and GPU tests share."""
import ctypes as C
import os

import numpy as np

import harness_build
from noise_host.pynoise import Refused, bits_equal  # noqa: F401  (the tests' names for them)
from spicey_amd import abi
from spicey_amd import tran_mc as tm

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SENTINEL = -7.25
SENTINEL_I = -99
REDUCE_NI = (1, 2, 63, 64, 65, 1000, 1024, 1025)
REDUCE_NS = (1, 5)
CASES = ("plain", "all_nan", "all_invalid_but_one", "ties", "third_invalid")
THREADS = (64, 192, 1024)
PROBS = (0.0, 0.01, 0.5, 0.99, 1.0)


def lib():
    global _LIB
    if _LIB is None:
        L = harness_build.load(HERE, "libspicey_tran_mc_host.so")
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.spicey_tmc_host_workspace_bytes.restype = i64
        L.spicey_tmc_host_workspace_bytes.argtypes = [i32, i32, i32, i32, i32]
        L.spicey_tmc_host_keys.restype = None
        L.spicey_tmc_host_keys.argtypes = [vp, i64, vp, vp]
        L.spicey_tmc_host_draw.restype = i32
        L.spicey_tmc_host_draw.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, C.c_char_p, i32]
        L.spicey_tmc_host_reduce.restype = i32
        L.spicey_tmc_host_reduce.argtypes = [i32, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i64, i32, C.c_char_p, i32]
        assert L.spicey_tmc_host_req_bytes() == C.sizeof(abi.SpiceyTranMcReq) and L.spicey_tmc_host_scalar_bytes() == abi.MC_SCALAR_DTYPE.itemsize
        _LIB = L
    return _LIB


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def keys(x):
    """(keys uint64, the doubles the keys decode to) of the harness for doubles x."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    k, back = np.zeros(x.shape, np.uint64), np.zeros(x.shape)
    lib().spicey_tmc_host_keys(x.ctypes.data, x.size, k.ctypes.data, back.ctypes.data)
    return k, back


def draw(R, Cv, Lv, tol, icdf, req, n_inst=None, nR=None, have_work=True, work_bytes=-1):
    """(R', C', L') of the harness — ohms, farads, henries — for nominal R / Cv / Lv [ni][n<kind>], tol [nE], icdf and a request
    abi.tran_mc_req(...).  A refusal raises Refused with the judge's text, after checking that the results kept their sentinel."""
    ni0 = np.asarray(R).shape[0]
    R, Cv, Lv = (np.ascontiguousarray(a, dtype=np.float64).reshape(ni0, -1) for a in (R, Cv, Lv))
    tol = None if tol is None else np.ascontiguousarray(tol, dtype=np.float64)
    icdf = None if icdf is None else np.ascontiguousarray(icdf, dtype=np.float64)
    oR, oC, oL = (np.full(a.shape, SENTINEL) for a in (R, Cv, Lv))
    err = C.create_string_buffer(256)
    rc = lib().spicey_tmc_host_draw(ni0 if n_inst is None else n_inst, R.shape[1] if nR is None else nR, Cv.shape[1], Lv.shape[1], _ptr(R), _ptr(Cv), _ptr(Lv),
                                    None if tol is None else tol.ctypes.data, None if icdf is None else icdf.ctypes.data,
                                    C.addressof(req) if req is not None else None, _ptr(oR), _ptr(oC), _ptr(oL), int(have_work), work_bytes, err, 256)
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and (oR == SENTINEL).all() and (oC == SENTINEL).all() and (oL == SENTINEL).all()
        raise Refused(err.value.decode())
    return oR, oC, oL


def rows_struct(rows, strides=abi.MC_PASS_STRIDE, n_rows=None):
    """(abi.SpiceyMcRows * 3, the arrays kept alive) of rows = (measure, timing, power), each [ni][n_rows][stride] or None."""
    arr, keep = (abi.SpiceyMcRows * 3)(), []
    for p, r in enumerate(rows):
        if r is None:
            arr[p].d_rows, arr[p].n_rows, arr[p].stride = None, 0 if n_rows is None else n_rows[p], strides[p]
            continue
        r = np.ascontiguousarray(r, dtype=np.float64)
        keep.append(r)
        arr[p].d_rows, arr[p].n_rows, arr[p].stride = r.ctypes.data, r.shape[1] if n_rows is None else n_rows[p], r.shape[2] if strides is abi.MC_PASS_STRIDE else strides[p]
    return arr, keep


def reduce(rows, scalars, valid=None, lo=None, hi=None, probs=(), n_inst=None, n_scalar=None, have_out=True, work_bytes=-1, threads=0, strides=abi.MC_PASS_STRIDE,
           n_rows=None, have_probs=True, have_rows=True):
    """(x [ni][ns], stat [ns][8 + 2 n_prob], sample [ni][2] int64) of the harness.  threads: of the sorting workgroup (0: the
    launcher's choice).  A refusal raises Refused, after checking that the results kept their sentinel."""
    ni0 = next(np.asarray(r).shape[0] for r in rows if r is not None)
    sc = np.ascontiguousarray(scalars, dtype=abi.MC_SCALAR_DTYPE).reshape(-1)
    ns = len(sc)
    arr, keep = rows_struct(rows, strides, n_rows)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
    hi = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
    probs = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    x = np.full((ni0, max(ns, 1)), SENTINEL)
    stat = np.full((max(ns, 1), abi.TRAN_MC_STAT_HEAD + 2 * len(probs)), SENTINEL)
    sample = np.full((ni0, 2), SENTINEL_I, np.int64)
    err = C.create_string_buffer(256)
    with np.errstate(all="ignore"):
        rc = lib().spicey_tmc_host_reduce(ni0 if n_inst is None else n_inst, C.addressof(arr) if have_rows else None, _ptr(sc), ns if n_scalar is None else n_scalar,
                                          None if valid is None else valid.ctypes.data, None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data,
                                          _ptr(probs) if have_probs else None, len(probs), x.ctypes.data, stat.ctypes.data, sample.ctypes.data, int(have_out),
                                          work_bytes, threads, err, 256)
    del keep
    if rc != abi.OK:
        assert rc == abi.ERR_BAD_DESC and (x == SENTINEL).all() and (stat == SENTINEL).all() and (sample == SENTINEL_I).all()
        raise Refused(err.value.decode())
    return x, stat, sample


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
def rows_like(ni, seed, n_meas=3, n_tim=2, n_pow=2):
    """Seeded rows (measure [ni][n_meas][8], timing [ni][n_tim][8], power [ni][n_pow][16]) with signs, zeros of both signs,
    infinities, denormals and NaNs among them."""
    rng = np.random.default_rng(seed)
    out = []
    for n, stride in ((n_meas, 8), (n_tim, 8), (n_pow, abi.POWER_ROW)):
        r = rng.normal(0.0, 1.0, (ni, n, stride)) * 10.0 ** rng.uniform(-3, 3, (ni, n, stride))
        flat = r.reshape(-1)
        pick = rng.integers(0, flat.size, max(flat.size // 9, 6))
        flat[pick] = rng.choice([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1.0, 1.0, -1.0], len(pick))
        out.append(r)
    return tuple(out)


def programs_like(n_scalar):
    """n_scalar programs over rows_like's shapes: a field, guarded fields, a quotient that divides by zero somewhere, a deep
    one, the longest one."""
    F, K, ADD, SUB, MUL, DIV, GUARD = tm.F, tm.K, tm.ADD, tm.SUB, tm.MUL, tm.DIV, tm.GUARD
    long = [F(2, 1, 4)]
    while len(long) + 2 <= abi.MC_SCALAR_INS:
        long += [K(1.5), MUL] if len(long) % 4 == 1 else [K(0.25), SUB]
    pool = [[F(0, 2, 7)],
            [F(1, 0, 0), GUARD, F(1, 0, 1)],
            [F(2, 0, 4), F(2, 1, 15), DIV],
            [F(0, 0, 0), F(0, 0, 1), F(0, 1, 2), F(1, 1, 3), ADD, MUL, SUB, K(-0.5), MUL],
            long,
            [F(0, 1, 4), K(2.0), SUB, GUARD, F(0, 1, 5), F(0, 1, 6), SUB]]
    return tm.make_scalars([pool[j % len(pool)] for j in range(n_scalar)])


def case_inputs(case, ni, ns, seed):
    """(rows, scalars, valid, lo, hi) of a named reduction case."""
    rows = [r.copy() for r in rows_like(ni, seed)]
    scalars = programs_like(ns)
    rng = np.random.default_rng(seed + 77)
    valid = None
    if case == "all_nan":
        rows[0][:, 2, 7] = np.nan  # what scalar 0 reads
    elif case == "all_invalid_but_one":
        valid = np.zeros(ni, np.uint8)
        valid[ni // 2] = 1
    elif case == "ties":
        rows[0][:, 2, 7] = np.where(rng.random(ni) < 0.5, -2.0, 3.0)  # ties for min and max
        rows[0][ni // 3, 2, 7] = 0.0
    elif case == "third_invalid":
        valid = np.ones(ni, np.uint8)
        valid[::3] = 0
    lo = np.where(rng.random(ns) < 0.3, -np.inf, -1.0)
    hi = np.where(rng.random(ns) < 0.3, np.inf, 10.0)
    return tuple(rows), scalars, valid, lo, hi


def draw_inputs(ni, shape, log2K, seed):
    from mc_host.pymc import draw_inputs as d
    return d(ni, shape, log2K, seed)


def drawn_flat(flat, tol, icdf, req):
    """A FlatCircuit whose value rows are the numpy draw's (ohms, farads, henries): what a Monte Carlo run's transient reads."""
    from mc_host.pymc import replicate_rows
    from spicey_amd.mc import mc_gains
    out = replicate_rows(flat)
    g = mc_gains(out.n_inst, tol, icdf, req.log2K, req.seed, bool(req.keep_first))
    nR, nC = out.nR, out.nC
    out.R_val = np.ascontiguousarray(out.R_val * g[:, :nR])
    out.C_val = np.ascontiguousarray(out.C_val * g[:, nR:nR + nC])
    out.L_val = np.ascontiguousarray(out.L_val * g[:, nR + nC:])
    return out


def flat_row(flat, k):
    """Instance k of `flat` as a FlatCircuit of one instance."""
    arrays = {key: getattr(flat, key) for key in abi.FlatCircuit.TOPO}
    for key in abi.FlatCircuit.VALS + ("S_ison",):
        arrays[key] = np.ascontiguousarray(getattr(flat, key)[k:k + 1])
    arrays["out_nodes"] = flat.out_nodes
    return abi.FlatCircuit(flat.n_nodes, 1, **arrays)


def reference_rows(out_v, out_i, reqs, treqs, preqs, dt):
    """The rows of the measure, timing and power passes in numpy (None for an empty list)."""
    from spicey_amd import measure as M
    return (M.reduce_reference(out_v, out_i, reqs, dt) if len(reqs) else None, M.reduce_reference_timing(out_v, out_i, treqs, dt) if len(treqs) else None,
            M.reduce_reference_power(out_v, out_i, preqs, dt) if len(preqs) else None)


def run_mc_reference(run, flat, steps, dt, src, req, tol, icdf, scalars, lo, hi, probs, reqs=(), treqs=(), preqs=(), reducer=None):
    """What Handle.run_mc returns, from `run(flat)` -> {out_v, out_i, inst_status, status, ...} of the drawn circuits (a second
    handle's run_reduced rows via `rows` in the result, or waveforms reduced here in numpy) and `reducer` (default: the harness)."""
    res = run(drawn_flat(flat, tol, icdf, req))
    ist = np.asarray(res["inst_status"])
    valid = (ist == 0).astype(np.uint8)
    out = {"status": res["status"], "detail": res.get("detail", ""), "inst_status": ist, "run": res, "state": res.get("state")}
    rows = res["rows"] if "rows" in res else reference_rows(res["out_v"], res.get("out_i"), reqs, treqs, preqs, dt)
    if valid.any():
        v = None if valid.all() else valid
        if reducer is None:
            out["x"], out["stat"], out["sample"] = reduce(rows, scalars, v, lo, hi, probs)
        else:
            out["x"] = tm.eval_reference_scalars(scalars, rows, v)
            out["sample"], out["stat"] = tm.reduce_reference_tran_mc(out["x"], v, lo, hi, probs)
    return out


class HostTranMcBackend:
    """run_tran_mc of a backend on the CPU: the numpy draw, the oracle's transient per drawn variant, the numpy rows of the
    passes, the harness's scalars and reduction."""

    def run_tran_mc(self, flat, steps, dt, src, req, tol, icdf, scalars, lo=None, hi=None, probs=(), reqs=(), treqs=(), preqs=(), want_x=False):
        from oracle.pyoracle import OracleBackend

        def run(drawn):
            parts = [OracleBackend().run(flat_row(drawn, k), steps, dt, src) for k in range(drawn.n_inst)]
            ist = np.array([p["status"] for p in parts], np.int32)
            bad = [p for p in parts if p["status"] != abi.OK]
            return {"status": bad[0]["status"] if bad else abi.OK, "detail": bad[0]["detail"] if bad else "", "inst_status": ist,
                    "out_v": np.concatenate([p["out_v"] for p in parts]), "out_i": np.concatenate([p["out_i"] for p in parts])}

        return run_mc_reference(run, flat, steps, dt, src, req, tol, icdf, scalars, lo, hi, probs, reqs, treqs, preqs)
