"""What the struct entry points of the reduced-run driver (spicey_run_reduced, spicey_run_mc, spicey_run_sens, spicey_run_levels)
and spicey_run_measure_spectrum refuse, with which text, in which order, and what a refusal leaves behind: of two faults the
earlier step's text, the caller's arrays untouched, no per-instance answer (spicey_last_inst_status = -1), the study's time
readouts at 0 (a header refusal returns before they are reset and leaves them as they were), and an accepted call on the same
handle right after it with the times of exactly the passes that ran.  The order inside a study call: the struct header, the
study's null result buffer, a list the study does not reduce, a negative count, every list empty, the run arguments, the passes'
judges in pass order, the study's judges (draw or design, then scalars or reduction), the structurally singular matrix.
One RC circuit on 1, 4 (Monte Carlo) and 3 (sensitivity, levels: nA = 1) instances, 8 steps; a refusal launches nothing."""
import ctypes as C

import numpy as np
import pytest

from spicey_amd import abi
from spicey_amd import tran_mc as tm
from spicey_amd.measure import make_four_reqs, make_power_reqs, make_reqs, make_spec_reqs, make_timing_reqs
from spicey_amd.netlist import parseNetlist

pytestmark = pytest.mark.gpu

RC = "* pulse into RC\nV1 in 0 PULSE(0 1 0 1u 1u 2u 4u)\nR1 in out 1k\nC1 out 0 1n\n.tran 1u 8u\n.end\n"
VLOOP = "* two sources across one node pair\nV1 in 0 PULSE(0 1 0 1u 1u 2u 4u)\nV2 in 0 PULSE(0 1 0 1u 1u 2u 4u)\nR1 in out 1k\nC1 out 0 1n\n.tran 1u 8u\n.end\n"
STEPS, DT, SENTINEL = 8, 1e-6, -7.25


def E(col=0, level=0.5, n=1):
    return (0, col, -1, 1, n, 0, 0, -1, level)


OK_M = make_reqs([(abi.MEAS_STATS, 0, 0, -1, 0, -1, 0.0, 0)])
BAD_M = make_reqs([(abi.MEAS_STATS, 0, 99, -1, 0, -1, 0.0, 0)])
OK_F = make_four_reqs([(0, 0, -1, 1, 0, -1, 1.0 / (4 * DT))])
OK_T = make_timing_reqs([(0, -1, None, E(), 0)])
BAD_T = make_timing_reqs([(0, -1, None, E(n=0), 0)])
OK_S = make_spec_reqs([(0, 0, -1, 0, 1, 3, 0, 0, 4)])
BAD_S = make_spec_reqs([(0, 0, -1, 0, 1, 14, 0, 0, 4)])
OK_P = make_power_reqs([(0, 0, -1, 0, 0, -1, 0, 0, -1)])
BAD_P = make_power_reqs([(0, 0, -1, 0, 0, -1, 2, 0, -1)])
SPEC_ROW = abi.spec_row_doubles(OK_S)
OK_SC, BAD_SC = tm.make_scalars([[tm.F(0, 0, 1)]]), tm.make_scalars([[tm.F(0, 99, 1)]])  # (measure row 0's field 1; a row that is not there)
TOL, UNI, PROBS = np.array([0.01, 0.02]), np.array([-1.0, 1.0]), np.array([0.5])
ACT, STEP, LVL = np.array([0], np.int32), np.array([0.01]), np.array([[0, 0], [1, -1], [-1, 1]], np.int8)

RUN_ARGS = "bad run arguments"
PER_INST = "src_per_inst must be 0 (one shared table) or 1 (one table per instance)"
COUNTS = "reduced: every count must be >= 0"
EMPTY = "reduced: every list is empty (at least one count must be > 0)"
MEAS_LIST = "measure: request 0: column out of range"
TIM_LIST = "timing: request 0: targ: n must not be 0"
POWER_LIST = "power: request 0: neg must be 0 or 1"
SPEC_ENTRY = "spectrum: n_req, n_four and n_timing must be >= 0, and meas / four / timing not null when their count is > 0"
SPEC_COUNT = "spectrum: n_req must be >= 1 and the request list not null"
STRUCTURAL = "singular at inst 0 step 0 iter 0 (structurally singular matrix)"
HEADER = {"reduced": ("reduced: lists must not be null", "reduced: struct_bytes is smaller than sizeof(SpiceyReducedLists)", "reduced: reserved must be 0"),
          "mc": ("tran mc: lists must not be null", "tran mc: lists.struct_bytes is smaller than sizeof(SpiceyReducedLists)", "tran mc: lists.reserved must be 0"),
          "sens": ("tran sens: lists must not be null", "tran sens: lists.struct_bytes is smaller than sizeof(SpiceyReducedLists)",
                   "tran sens: lists.reserved must be 0")}
NOT_REDUCED = {k: f"tran {k}: the fourier, spectrum and values lists are not reduced by this call (measure, timing and power are)" for k in ("mc", "sens")}
FIELD_ROW = {k: f"tran {k}: a FIELD's row is out of range" for k in ("mc", "sens")}
PASS_MS = ("measure", "fourier", "timing", "spectrum", "power", "values")
LISTS = (("meas", "reqs", "n_req"), ("four", "freqs", "n_four"), ("timing", "treqs", "n_timing"), ("spec", "sreqs", "n_spec"), ("power", "preqs", "n_power"),
         ("values", "vreqs", "n_values"))


def _handle(text, n):
    from spicey_amd.lib import Handle
    ckt = parseNetlist(text)
    return Handle(abi.flatten(ckt).replicate(n)), np.ascontiguousarray(abi.source_table(ckt, DT, STEPS), dtype=np.float64)


@pytest.fixture(scope="module")
def rc1():
    hs = _handle(RC, 1)
    yield hs
    hs[0].close()


@pytest.fixture(scope="module")
def rc4():
    hs = _handle(RC, 4)
    yield hs
    hs[0].close()


@pytest.fixture(scope="module")
def rc3():
    hs = _handle(RC, 3)
    yield hs
    hs[0].close()


def _lists(outs=None, **kw):
    """abi.SpiceyReducedLists of the lists named by result key (meas=OK_M, ...), their counts and the usual strides; any other
    keyword sets that field afterwards (n_req=-1, reserved=1, ...).  outs: the result arrays by key (a study takes none)."""
    a = abi.SpiceyReducedLists()
    a.struct_bytes, a.four_stride, a.spec_stride, a.values_stride = C.sizeof(a), 3, SPEC_ROW, 1
    keep, null_out = [], kw.pop("null_out", ())
    for key, lst, cnt in LISTS:
        recs = kw.pop(key, None)
        if recs is not None:
            keep.append(recs.copy())
            setattr(a, lst, keep[-1].ctypes.data)
            setattr(a, cnt, len(recs))
            setattr(a, key, outs[key].ctypes.data if outs and key not in null_out else None)
    for field, value in kw.items():
        setattr(a, field, value)
    return a, keep


def _ptr(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _addr(a):
    return a.ctypes.data if a is not None else None


def _raw(hs, fn, bufs, lists, steps, per_inst, mid, tail):
    """fn(handle, steps, DT, src, per_inst, lists, *mid, *tail's arrays, iters) -> (status, text, the arrays are as they were)."""
    h, src = hs
    bufs["iters"] = np.full((h.flat.n_inst, STEPS + 1), -5, np.int32)
    was = {k: b.copy() for k, b in bufs.items()}
    status = fn(h.h, steps, DT, _ptr(src), per_inst, C.addressof(lists[0]) if lists is not None else None, *mid, *tail, _ptr(bufs["iters"], C.c_int32))
    return status, h.error(), all(np.array_equal(bufs[k], was[k]) for k in was)


def _mc(hs, lists, steps=STEPS, per_inst=0, req=abi.tran_mc_req(0, True, 3), tol=TOL, icdf=UNI, scalars=OK_SC, n_scalar=1, lo=None, probs=PROBS, null=()):
    ni = hs[0].flat.n_inst
    bufs = {"stat": np.full((1, abi.TRAN_MC_STAT_HEAD + 2 * len(PROBS)), SENTINEL), "sample": np.full((ni, 2), -9, np.int64), "x": np.full((ni, 1), SENTINEL)}
    mid = (C.addressof(req) if req is not None else None, _ptr(tol), _ptr(icdf), _addr(scalars), n_scalar, _ptr(lo), None, _ptr(probs), len(probs))
    tail = (None if "stat" in null else _ptr(bufs["stat"]), None if "sample" in null else _ptr(bufs["sample"], C.c_int64), _ptr(bufs["x"]))
    return _raw(hs, hs[0].L.spicey_run_mc, bufs, lists, steps, per_inst, mid, tail)


def _sens(hs, lists, steps=STEPS, per_inst=0, req=abi.tran_sens_req(abi.TS_ONE_AT_A_TIME, 1), act=ACT, step=STEP, tol=TOL, scalars=OK_SC, n_scalar=1, null=()):
    bufs = {"sens": np.full((1, 1, 2), SENTINEL), "sign": np.full((1, 1), 5, np.int8), "bound": np.full((1, abi.TRAN_SENS_BOUND_ROW), SENTINEL),
            "x": np.full((3, 1), SENTINEL)}
    mid = (C.addressof(req) if req is not None else None, _addr(act), _ptr(step), _ptr(tol), _addr(scalars), n_scalar)
    tail = tuple(None if k in null else (_addr(bufs[k]) if k == "sign" else _ptr(bufs[k])) for k in ("sens", "sign", "bound", "x"))
    return _raw(hs, hs[0].L.spicey_run_sens, bufs, lists, steps, per_inst, mid, tail)


def _levels(hs, lists, steps=STEPS, per_inst=0, req=abi.tran_sens_req(abi.TS_LEVELS, 0), lvl=LVL, tol=TOL, scalars=OK_SC, n_scalar=1, null=()):
    bufs = {"x": np.full((3, 1), SENTINEL)}
    mid = (C.addressof(req) if req is not None else None, _addr(lvl), _ptr(tol), _addr(scalars), n_scalar)
    return _raw(hs, hs[0].L.spicey_run_levels, bufs, lists, steps, per_inst, mid, (None if "x" in null else _ptr(bufs["x"]),))


def _reduced(hs, lists, steps=STEPS, per_inst=0):
    return _raw(hs, hs[0].L.spicey_run_reduced, lists[2] if lists is not None else {}, lists, steps, per_inst, (), ())


def _reduced_lists(**kw):
    outs = {"meas": np.full((1, 1, 8), SENTINEL), "timing": np.full((1, 1, 8), SENTINEL), "power": np.full((1, 1, abi.POWER_ROW), SENTINEL)}
    return _lists(outs, **kw) + (outs,)


def _study_ms(h):
    return (h.L.spicey_last_tran_mc_ms(h.h), h.L.spicey_last_tran_mc_draw_ms(h.h), h.L.spicey_last_tran_sens_ms(h.h), h.L.spicey_last_tran_sens_design_ms(h.h))


def _refused(hs, call, text, lists, header=False, status=abi.ERR_BAD_DESC, **kw):
    h = hs[0]
    ni, before = h.flat.n_inst, _study_ms(h)
    got, detail, untouched = call(hs, lists, **kw)
    assert got == status and detail == text, (got, detail)
    assert untouched, text
    # no per-instance answer after a refusal, except the structural one: every instance then failed
    ist = np.full(ni, -3, np.int32)
    bad = h.L.spicey_last_inst_status(h.h, _ptr(ist, C.c_int32))
    assert (bad == ni and (ist == abi.ERR_SINGULAR).all()) if status == abi.ERR_SINGULAR else (bad == -1 and (ist == -3).all()), (text, bad, ist)
    if call is not _reduced:
        assert _study_ms(h) == (before if header else (0.0, 0.0, 0.0, 0.0)), text


def _passes_that_ran(h, ran):
    times = {k: getattr(h.L, f"spicey_last_{k}_ms")(h.h) for k in PASS_MS}
    assert all((times[k] > 0) if k in ran else (times[k] == 0.0) for k in PASS_MS), (ran, times)


def _accepted(hs, kind):
    """The Handle method of the study right after a refusal: it works, the study's two times and exactly its passes' are > 0."""
    h, src = hs
    if kind == "mc":
        res = h.run_mc(STEPS, DT, src, abi.tran_mc_req(0, True, 3), TOL, UNI, OK_SC, probs=PROBS, reqs=OK_M, treqs=OK_T, want_x=True)
        ran, ms = ("measure", "timing"), ("mc_ms", "draw_ms")
        assert (res["stat"][:, 0] == h.flat.n_inst).all()
    elif kind == "sens":
        res = h.run_sens(STEPS, DT, src, abi.tran_sens_req(abi.TS_ONE_AT_A_TIME, 1), ACT, STEP, TOL, OK_SC, reqs=OK_M, preqs=OK_P, want_x=True)
        ran, ms = ("measure", "power"), ("sens_ms", "design_ms")
        assert res["sens"].shape == (1, 1, 2) and np.isfinite(res["bound"][:, 0]).all()
    else:
        res = h.run_levels(STEPS, DT, src, abi.tran_sens_req(abi.TS_LEVELS, 0), LVL, TOL, OK_SC, reqs=OK_M)
        ran, ms = ("measure",), ("sens_ms", "design_ms")
    assert res["status"] == abi.OK and res["detail"] == "" and (res["inst_status"] == 0).all() and res["kernel_ms"] > 0
    assert res[ms[0]] > 0 and res[ms[1]] > 0 and np.isfinite(res["x"]).all()
    want = _study_ms(h)
    assert (res[ms[0]], res[ms[1]]) == (want[:2] if kind == "mc" else want[2:]) and (want[2:] if kind == "mc" else want[:2]) == (0.0, 0.0)
    _passes_that_ran(h, ran)


def _header_and_lists(hs, call, kind, accepted):
    """Steps 1 to 6 of a study call, which the three studies share; `kind` names the texts' prefix."""
    null, small, reserved = HEADER[kind]
    buffer = f"tran {kind}: null buffer"
    first = {"mc": "stat", "sens": "bound"}.get(kind if call is not _levels else "levels", "x")
    for again in (False, True):  # (on the fresh handle, then behind an accepted call: the readouts stay as that call left them)
        _refused(hs, call, null, None, header=True, null=(first,))                                         # 1 before 2
        _refused(hs, call, small, _lists(meas=OK_M, struct_bytes=C.sizeof(abi.SpiceyReducedLists) - 1, reserved=1), header=True)
        _refused(hs, call, small, _lists(meas=OK_M, struct_bytes=0), header=True)
        _refused(hs, call, reserved, _lists(meas=OK_M, four=OK_F, reserved=1), header=True, null=(first,))
        if not again:
            accepted()
    _refused(hs, call, buffer, _lists(meas=OK_M, four=OK_F), null=(first,))                                # 2 before 3
    for lst in (dict(four=OK_F), dict(spec=OK_S), dict(n_values=1)):
        _refused(hs, call, NOT_REDUCED[kind], _lists(meas=OK_M, n_req=-1, **lst))                          # 3 before 4
    for cnt in ("n_req", "n_timing", "n_power"):
        _refused(hs, call, COUNTS, _lists(**{cnt: -1}), steps=-1)                                          # 4 before 5 and 6
    _refused(hs, call, COUNTS, _lists(meas=OK_M, n_four=-1))
    _refused(hs, call, EMPTY, _lists(), steps=-1)                                                          # 5 before 6
    _refused(hs, call, EMPTY, _lists(reqs=OK_M.ctypes.data), per_inst=2)
    _refused(hs, call, RUN_ARGS, _lists(meas=BAD_M), steps=-1, per_inst=2)                                 # 6 before 7
    _refused(hs, call, PER_INST, _lists(meas=BAD_M), per_inst=2)
    _refused(hs, call, PER_INST, _lists(meas=OK_M), per_inst=-1, scalars=BAD_SC)
    accepted()


def _pass_order(hs, call, first_study_text, **first_study_fault):
    """Step 7, and that it comes before step 8: measure before timing before power before the study's first judge."""
    _refused(hs, call, MEAS_LIST, _lists(meas=BAD_M, timing=BAD_T, power=BAD_P), **first_study_fault)
    _refused(hs, call, TIM_LIST, _lists(meas=OK_M, timing=BAD_T, power=BAD_P), **first_study_fault)
    _refused(hs, call, POWER_LIST, _lists(meas=OK_M, timing=OK_T, power=BAD_P), **first_study_fault)
    _refused(hs, call, POWER_LIST, _lists(power=BAD_P), **first_study_fault)
    _refused(hs, call, first_study_text, _lists(meas=OK_M, timing=OK_T, power=OK_P), **first_study_fault)


def test_run_mc(rc4):
    _header_and_lists(rc4, _mc, "mc", lambda: _accepted(rc4, "mc"))
    for k in ("stat", "sample"):
        _refused(rc4, _mc, "tran mc: null buffer", _lists(meas=OK_M, spec=OK_S), null=(k,))
    bad_req = abi.tran_mc_req(0, True, 3)
    bad_req.reserved = 1
    _pass_order(rc4, _mc, "tran mc: reserved must be 0", req=bad_req)
    # 8: the draw's judge (request, buffers, table, tolerances) before the reduction's (counts, buffers, programs, probabilities, limits)
    ok = dict(meas=OK_M, timing=OK_T)
    _refused(rc4, _mc, "tran mc: null request", _lists(**ok), req=None, scalars=BAD_SC)
    _refused(rc4, _mc, "tran mc: log2K outside [0, 12]", _lists(**ok), req=abi.tran_mc_req(13, True, 3), tol=None)
    _refused(rc4, _mc, "tran mc: null buffer", _lists(**ok), tol=None, scalars=BAD_SC)
    _refused(rc4, _mc, "tran mc: null buffer", _lists(**ok), icdf=None, n_scalar=0)
    _refused(rc4, _mc, "tran mc: the table must be finite and non-decreasing", _lists(**ok), icdf=np.array([1.0, -1.0]), tol=np.array([0.01, -0.1]))
    _refused(rc4, _mc, "tran mc: a tolerance must be finite and >= 0", _lists(**ok), tol=np.array([0.01, -0.1]), scalars=BAD_SC)
    _refused(rc4, _mc, "tran mc: tol * max|icdf| >= 1: a drawn value could be zero or negative", _lists(**ok), tol=np.array([0.01, 1.0]), scalars=BAD_SC)
    _refused(rc4, _mc, "tran mc: bad counts (n_inst, n_scalar >= 1, n_prob >= 0)", _lists(**ok), n_scalar=0, scalars=None)
    _refused(rc4, _mc, "tran mc: null buffer", _lists(**ok), scalars=None, probs=np.array([1.5]))
    _refused(rc4, _mc, FIELD_ROW["mc"], _lists(**ok), scalars=BAD_SC, probs=np.array([1.5]))
    _refused(rc4, _mc, "tran mc: a FIELD names a pass whose list is empty", _lists(timing=OK_T))
    _refused(rc4, _mc, "tran mc: a probability outside [0, 1]", _lists(**ok), probs=np.array([1.5]), lo=np.array([np.nan]))
    _refused(rc4, _mc, "tran mc: a limit is NaN", _lists(**ok), lo=np.array([np.nan]))
    _accepted(rc4, "mc")


def test_run_sens(rc3):
    _header_and_lists(rc3, _sens, "sens", lambda: _accepted(rc3, "sens"))
    for k in ("sens", "sign", "bound"):
        _refused(rc3, _sens, "tran sens: null buffer", _lists(meas=OK_M, four=OK_F), null=(k,))
    bad_req = abi.tran_sens_req(abi.TS_ONE_AT_A_TIME, 1)
    bad_req.reserved[1] = 1
    _pass_order(rc3, _sens, "tran sens: reserved must be 0", req=bad_req)
    # 8: the design's judge, then the tolerances (null, then their values), then the scalars' and the reduction's
    ok = dict(meas=OK_M, power=OK_P)
    bad_tol = np.array([0.01, 1.0])
    _refused(rc3, _sens, "tran sens: this call takes the ONE_AT_A_TIME design", _lists(**ok), req=abi.tran_sens_req(abi.TS_LEVELS, 0), tol=None)
    _refused(rc3, _sens, "tran sens: ONE_AT_A_TIME needs n_inst = 1 + 2 nA", _lists(**ok), req=abi.tran_sens_req(abi.TS_ONE_AT_A_TIME, 2), tol=None)
    _refused(rc3, _sens, "tran sens: null buffer", _lists(**ok), act=None, tol=bad_tol)
    _refused(rc3, _sens, "tran sens: an active element is out of range", _lists(**ok), act=np.array([2], np.int32), tol=None)
    _refused(rc3, _sens, "tran sens: a step must be finite and in (0, 1)", _lists(**ok), step=np.array([1.0]), tol=None)
    _refused(rc3, _sens, "tran sens: null buffer", _lists(**ok), tol=None, scalars=BAD_SC)
    _refused(rc3, _sens, "tran sens: a tolerance must be finite and in [0, 1)", _lists(**ok), tol=bad_tol, scalars=BAD_SC)
    _refused(rc3, _sens, "tran sens: bad counts (n_inst, n_scalar >= 1, n_prob >= 0)", _lists(**ok), n_scalar=0)
    _refused(rc3, _sens, FIELD_ROW["sens"], _lists(**ok), scalars=BAD_SC)
    _accepted(rc3, "sens")


def test_run_levels(rc3):
    _header_and_lists(rc3, _levels, "sens", lambda: _accepted(rc3, "levels"))
    bad_req = abi.tran_sens_req(abi.TS_LEVELS, 0)
    bad_req.reserved[0] = 1
    _pass_order(rc3, _levels, "tran sens: reserved must be 0", req=bad_req)
    # 8: the design's judge (request, arrays, tolerances, levels), then the scalars'
    ok = dict(meas=OK_M, timing=OK_T)
    bad_lvl = LVL.copy()
    bad_lvl[2, 1] = 2
    _refused(rc3, _levels, "tran sens: this call takes the LEVELS design", _lists(**ok), req=abi.tran_sens_req(abi.TS_ONE_AT_A_TIME, 1), scalars=BAD_SC)
    _refused(rc3, _levels, "tran sens: LEVELS needs nA = 0", _lists(**ok), req=abi.tran_sens_req(abi.TS_LEVELS, 1), lvl=None)
    _refused(rc3, _levels, "tran sens: null buffer", _lists(**ok), lvl=None, scalars=BAD_SC)
    _refused(rc3, _levels, "tran sens: null buffer", _lists(**ok), tol=None, scalars=BAD_SC)
    _refused(rc3, _levels, "tran sens: a tolerance must be finite and in [0, 1)", _lists(**ok), tol=np.array([0.01, 1.0]), lvl=bad_lvl)
    _refused(rc3, _levels, "tran sens: a level must be -1, 0 or +1", _lists(**ok), lvl=bad_lvl, scalars=BAD_SC)
    _refused(rc3, _levels, "tran sens: null buffer", _lists(**ok), scalars=None)
    _refused(rc3, _levels, FIELD_ROW["sens"], _lists(**ok), scalars=BAD_SC)
    _accepted(rc3, "levels")
    # the two entry points share the readouts: each accepted call writes both, each refusal behind the header resets both
    _accepted(rc3, "sens")
    _refused(rc3, _levels, FIELD_ROW["sens"], _lists(**ok), scalars=BAD_SC)
    _accepted(rc3, "levels")


def test_the_structural_refusal_comes_last():
    """9: a matrix that is singular by its structure is refused behind every judge, before any launch, and answers for every instance."""
    for n, call, kind, fault in ((4, _mc, "mc", dict(scalars=BAD_SC)), (3, _sens, "sens", dict(scalars=BAD_SC)), (3, _levels, "sens", dict(scalars=BAD_SC))):
        hs = _handle(VLOOP, n)
        try:
            _refused(hs, call, FIELD_ROW[kind], _lists(meas=OK_M), **fault)
            _refused(hs, call, MEAS_LIST, _lists(meas=BAD_M))
            _refused(hs, call, STRUCTURAL, _lists(meas=OK_M), status=abi.ERR_SINGULAR)
            _refused(hs, call, EMPTY, _lists())  # (and the next refusal forgets that answer)
        finally:
            hs[0].close()


def test_run_reduced_header(rc1):
    null, small, reserved = HEADER["reduced"]
    _refused(rc1, _reduced, null, None, steps=-1)
    _refused(rc1, _reduced, small, _reduced_lists(meas=OK_M, struct_bytes=C.sizeof(abi.SpiceyReducedLists) - 1, reserved=1))
    _refused(rc1, _reduced, reserved, _reduced_lists(meas=OK_M, n_timing=-1, reserved=1))
    # behind the header: the counts, every list empty, the run arguments, a null result pointer, the lists in pass order
    _refused(rc1, _reduced, COUNTS, _reduced_lists(n_power=-1), steps=-1)
    _refused(rc1, _reduced, EMPTY, _reduced_lists(), steps=-1)
    _refused(rc1, _reduced, RUN_ARGS, _reduced_lists(meas=BAD_M), steps=-1)
    _refused(rc1, _reduced, "reduced: a result pointer is null where its count is > 0", _reduced_lists(meas=BAD_M, timing=OK_T, null_out=("timing",)))
    _refused(rc1, _reduced, MEAS_LIST, _reduced_lists(meas=BAD_M, timing=BAD_T))
    _refused(rc1, _reduced, TIM_LIST, _reduced_lists(meas=OK_M, timing=BAD_T, power=BAD_P))
    h, src = rc1
    res = h.run_reduced(STEPS, DT, src, reqs=OK_M, preqs=OK_P)
    assert res["status"] == abi.OK and res["detail"] == "" and res["meas"][0, 0, 1] > 0.5
    _passes_that_ran(h, ("measure", "power"))


class L4:
    """One list of a raw positional call: the records, the count the call states (default: their number) and whether it gets an out array."""

    def __init__(self, reqs, count=None, out=True):
        self.reqs, self.count, self.out = reqs, len(reqs) if count is None else count, out


def _spectrum(rc1, text, m, f, t, s, steps=STEPS):
    """spicey_run_measure_spectrum with exactly these counts and pointers is refused with `text` and writes nothing."""
    h, src = rc1
    outs = {"meas": np.full((1, 2, 8), SENTINEL), "four": np.full((1, 2, 3), SENTINEL), "timing": np.full((1, 2, 8), SENTINEL),
            "spec": np.full((1, 2, SPEC_ROW), SENTINEL), "iters": np.full((1, STEPS + 1), -5, np.int32)}
    args = [h.h, steps, DT, _ptr(src), 0]
    for lst, name in zip((m, f, t, s), ("meas", "four", "timing", "spec")):
        args += [_addr(lst.reqs) if len(lst.reqs) else None, lst.count, _ptr(outs[name]) if lst.out else None]
        if name in ("four", "spec"):
            args.append(3 if name == "four" else SPEC_ROW)
    status = h.L.spicey_run_measure_spectrum(*args, _ptr(outs["iters"], C.c_int32))
    assert status == abi.ERR_BAD_DESC and h.error() == text, (status, h.error())
    assert all((outs[k] == SENTINEL).all() for k in ("meas", "four", "timing", "spec")) and (outs["iters"] == -5).all(), text
    ist = np.full(1, -3, np.int32)
    assert h.L.spicey_last_inst_status(h.h, _ptr(ist, C.c_int32)) == -1 and ist[0] == -3, text


def test_run_measure_spectrum_entry_text(rc1):
    ok = (L4(OK_M), L4(OK_F), L4(OK_T))
    # behind the run arguments, which are judged against `spec`, this entry point's own out array
    _spectrum(rc1, RUN_ARGS, L4(OK_M, count=-1), L4(OK_F), L4(OK_T), L4(OK_S, out=False))
    _spectrum(rc1, RUN_ARGS, L4(OK_M), L4(OK_F, out=False), L4(OK_T), L4(OK_S), steps=-1)
    # a negative count or a null out pointer with a positive count in any earlier list — before any list is read, its own included
    for k in range(3):
        for fault in (dict(count=-1), dict(out=False)):
            lists = [L4(lst.reqs, **fault) if j == k else lst for j, lst in enumerate(ok)]
            _spectrum(rc1, SPEC_ENTRY, *lists, L4(BAD_S))
            _spectrum(rc1, SPEC_ENTRY, *lists, L4(OK_S, count=0))
    _spectrum(rc1, SPEC_ENTRY, L4(BAD_M), L4(OK_F, count=-1), L4(OK_T), L4(OK_S))
    _spectrum(rc1, SPEC_ENTRY, L4(BAD_M, out=False), L4(OK_F), L4(BAD_T), L4(OK_S))
    _spectrum(rc1, MEAS_LIST, L4(BAD_M), L4(OK_F), L4(BAD_T), L4(BAD_S))
    _spectrum(rc1, TIM_LIST, L4(OK_M), L4(OK_F), L4(BAD_T), L4(BAD_S))
    _spectrum(rc1, "spectrum: request 0: log2n outside 3..13", *ok, L4(BAD_S))
    _spectrum(rc1, SPEC_COUNT, *ok, L4(OK_S, count=0))
    h, src = rc1
    res = h.run_measure_spectrum(STEPS, DT, src, OK_M, [], OK_T, OK_S)
    assert res["status"] == abi.OK and res["detail"] == "" and res["spec"].shape == (1, 1, SPEC_ROW) and res["spectrum_ms"] > 0
    _passes_that_ran(h, ("measure", "timing", "spectrum"))
