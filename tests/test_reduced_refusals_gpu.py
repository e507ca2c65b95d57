"""What the three reduced-run entry points (spicey_run_measure, spicey_run_measure_fourier, spicey_run_measure_timing) refuse,
in which order, and what they leave behind: the text and status of every refusal that depends on the entry point, the earlier
pass's text when two lists are at fault, the caller's arrays untouched, and an accepted call on the same handle right after
it with the pass times of exactly the passes that ran.  One one-instance RC circuit, 8 steps; a refusal launches nothing."""
import ctypes as C

import numpy as np
import pytest

from spicey_amd import abi
from spicey_amd.measure import make_four_reqs, make_reqs, make_timing_reqs
from spicey_amd.netlist import parseNetlist

pytestmark = pytest.mark.gpu

RC = "* pulse into RC\nV1 in 0 PULSE(0 1 0 1u 1u 2u 4u)\nR1 in out 1k\nC1 out 0 1n\n.tran 1u 8u\n.end\n"
STEPS, DT, SENTINEL = 8, 1e-6, -7.25


def E(col=0, level=0.5, n=1):
    return (0, col, -1, 1, n, 0, 0, -1, level)


OK_M = make_reqs([(abi.MEAS_STATS, 0, 0, -1, 0, -1, 0.0, 0)])
BAD_M = make_reqs([(abi.MEAS_STATS, 0, 99, -1, 0, -1, 0.0, 0)])
OK_F = make_four_reqs([(0, 0, -1, 1, 0, -1, 1.0 / (4 * DT))])
BAD_F = make_four_reqs([(0, 0, -1, 0, 0, -1, 1.0 / (4 * DT))])
OK_T = make_timing_reqs([(0, -1, None, E(), 0)])
BAD_T = make_timing_reqs([(0, -1, None, E(n=0), 0)])
NO_M, NO_F = make_reqs([]), make_four_reqs([])

RUN_ARGS = "bad run arguments"
MEAS_COUNT = "measure: n_req must be >= 1 and the request list not null"
FOUR_ENTRY = "fourier: n_req must be >= 0, and meas not null when n_req > 0"
TIM_ENTRY = "timing: n_req and n_four must be >= 0, and meas / four not null when their count is > 0"
MEAS_LIST = "measure: request 0: column out of range"
FOUR_LIST = "fourier: request 0: n_harm outside 1..16"
TIM_LIST = "timing: request 0: targ: n must not be 0"


@pytest.fixture(scope="module")
def rc():
    from spicey_amd.lib import Handle
    ckt = parseNetlist(RC)
    h = Handle(abi.flatten(ckt))
    yield h, np.ascontiguousarray(abi.source_table(ckt, DT, STEPS), dtype=np.float64)
    h.close()


class L3:
    """One list of a raw call: the records, the count the call states (default: their number) and whether it gets an out array."""

    def __init__(self, reqs, count=None, out=True):
        self.reqs, self.count, self.out = reqs, len(reqs) if count is None else count, out


def _raw(rc, entry, m, f=None, t=None):
    """Entry point `entry` (0, 1, 2) on the handle's library with exactly these counts and pointers -> (status, text, arrays)."""
    h, src = rc
    from spicey_amd.lib import _p, _reqs_ptr
    outs = {"meas": np.full((1, 2, 8), SENTINEL), "four": np.full((1, 2, 3), SENTINEL), "timing": np.full((1, 2, 8), SENTINEL),
            "iters": np.full((1, STEPS + 1), -5, np.int32)}
    args = [h.h, STEPS, DT, _p(src, C.c_double), 0]
    for lst, name in ((m, "meas"), (f, "four"), (t, "timing"))[:entry + 1]:
        args += [_reqs_ptr(lst.reqs), lst.count, _p(outs[name], C.c_double) if lst.out else None]
        if name == "four":
            args.append(3)
    fn = (h.L.spicey_run_measure, h.L.spicey_run_measure_fourier, h.L.spicey_run_measure_timing)[entry]
    status = fn(*args, _p(outs["iters"], C.c_int32))
    return status, h.error(), outs


def _refused(rc, text, entry, m, f=None, t=None):
    status, detail, outs = _raw(rc, entry, m, f, t)
    assert status == abi.ERR_BAD_DESC and detail == text, (entry, status, detail)
    assert all((outs[k] == SENTINEL).all() for k in ("meas", "four", "timing")) and (outs["iters"] == -5).all(), (entry, text)


def _accepted(rc, entry, reqs, freqs=None, treqs=None):
    """The Handle method of `entry` right after a refusal: it works, and exactly the passes that ran took time."""
    h, src = rc
    res = (h.run_measure(STEPS, DT, src, reqs) if entry == 0 else h.run_measure_fourier(STEPS, DT, src, reqs, freqs) if entry == 1
           else h.run_measure_timing(STEPS, DT, src, reqs, freqs, treqs))
    assert res["status"] == abi.OK and res["detail"] == "" and (res["inst_status"] == 0).all() and res["kernel_ms"] > 0
    ran = {"measure_ms": len(reqs) > 0, "fourier_ms": freqs is not None and len(freqs) > 0, "timing_ms": treqs is not None}
    times = {"measure_ms": h.L.spicey_last_measure_ms(h.h), "fourier_ms": h.L.spicey_last_fourier_ms(h.h), "timing_ms": h.L.spicey_last_timing_ms(h.h)}
    for k, on in ran.items():
        assert (times[k] > 0) if on else (times[k] == 0.0), (entry, k, times)
    keys = ("measure_ms", "fourier_ms", "timing_ms")[:entry + 1]
    assert all(res[k] == times[k] for k in keys) and not any(k in res for k in ("four", "fourier_ms", "timing", "timing_ms")[2 * entry:])
    assert res["meas"].shape == (1, len(reqs), 8) and (len(reqs) == 0 or res["meas"][0, 0, 1] > 0.5)  # (the pulse's top)
    return res


def test_run_measure(rc):
    _refused(rc, RUN_ARGS, 0, L3(OK_M, out=False))
    _refused(rc, MEAS_COUNT, 0, L3(OK_M, count=-1))
    _refused(rc, MEAS_COUNT, 0, L3(NO_M))
    _refused(rc, MEAS_LIST, 0, L3(BAD_M))
    _accepted(rc, 0, OK_M)


def test_run_measure_fourier(rc):
    # the run arguments are judged against `four`, this entry point's own last out array, and before anything else
    _refused(rc, RUN_ARGS, 1, L3(OK_M, count=-1), L3(OK_F, out=False))
    # its own refusals: a negative count, a null out pointer with a positive count — before either list is read
    _refused(rc, FOUR_ENTRY, 1, L3(OK_M, count=-1), L3(OK_F))
    _refused(rc, FOUR_ENTRY, 1, L3(BAD_M, out=False), L3(BAD_F))
    ref = _accepted(rc, 1, OK_M, OK_F)
    # two lists at fault: the earlier pass's text
    _refused(rc, MEAS_LIST, 1, L3(BAD_M), L3(BAD_F))
    _refused(rc, FOUR_LIST, 1, L3(OK_M), L3(BAD_F))
    _refused(rc, FOUR_LIST, 1, L3(NO_M, out=False), L3(BAD_F))
    only = _accepted(rc, 1, NO_M, OK_F)
    assert only["four"].shape == (1, 1, 3) and np.array_equal(only["four"], ref["four"])


def test_run_measure_timing(rc):
    _refused(rc, RUN_ARGS, 2, L3(OK_M, count=-1), L3(OK_F), L3(OK_T, out=False))
    for m, f in ((L3(OK_M, count=-1), L3(OK_F)), (L3(OK_M, out=False), L3(OK_F)), (L3(OK_M), L3(OK_F, count=-1)), (L3(OK_M), L3(OK_F, out=False)),
                 (L3(BAD_M, out=False), L3(BAD_F))):
        _refused(rc, TIM_ENTRY, 2, m, f, L3(BAD_T))
    ref = _accepted(rc, 2, OK_M, OK_F, OK_T)
    # faults in two or three lists: measure before fourier before timing
    _refused(rc, MEAS_LIST, 2, L3(BAD_M), L3(BAD_F), L3(BAD_T))
    _refused(rc, MEAS_LIST, 2, L3(BAD_M), L3(OK_F), L3(BAD_T))
    _refused(rc, FOUR_LIST, 2, L3(OK_M), L3(BAD_F), L3(BAD_T))
    _refused(rc, FOUR_LIST, 2, L3(NO_M, out=False), L3(BAD_F), L3(BAD_T))
    _refused(rc, TIM_LIST, 2, L3(OK_M), L3(OK_F), L3(BAD_T))
    _refused(rc, TIM_LIST, 2, L3(NO_M, out=False), L3(NO_F, out=False), L3(BAD_T))
    only = _accepted(rc, 2, NO_M, NO_F, OK_T)
    assert only["four"].shape == (1, 0, 1) and np.array_equal(only["timing"], ref["timing"]) and ref["timing"][0, 0, 3] >= 0  # (the edge was found)
    # the next entry point's call forgets the times of the passes it does not run
    assert np.array_equal(_accepted(rc, 1, OK_M, OK_F)["meas"], ref["meas"])
    assert np.array_equal(_accepted(rc, 0, OK_M)["meas"], ref["meas"])
