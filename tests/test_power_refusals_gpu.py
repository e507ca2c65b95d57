"""What spicey_run_measure_power, entry point 4 of the reduced run, refuses, in which order, and what it leaves behind: the
run arguments judged against `power`, its own text before any list is read, the earliest faulty list's text when several
lists are at fault, the caller's arrays untouched, and an accepted call on the same handle right after it with the pass
times of exactly the passes that ran.  One one-instance RC circuit, 8 steps; a refusal launches nothing."""
import ctypes as C

import numpy as np
import pytest

from spicey_amd import abi
from spicey_amd.measure import make_four_reqs, make_power_reqs, make_reqs, make_spec_reqs, make_timing_reqs
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
OK_S = make_spec_reqs([(0, 0, -1, 0, 1, 3, 0, 0, 4)])
BAD_S = make_spec_reqs([(0, 0, -1, 0, 1, 14, 0, 0, 4)])
# (every list reads v(in), the source's own waveform: the handle's state carries over from call to call, the source does not)
OK_P = make_power_reqs([(0, 0, -1, 0, 0, -1, 0, 0, -1)])  # v(in) v(in)
BAD_P = make_power_reqs([(0, 0, -1, 0, 0, -1, 2, 0, -1)])
NO_M, NO_F, NO_T, NO_S, NO_P = make_reqs([]), make_four_reqs([]), make_timing_reqs([]), make_spec_reqs([]), make_power_reqs([])

RUN_ARGS = "bad run arguments"
POWER_ENTRY = "power: n_req, n_four, n_timing and n_spec must be >= 0, and meas / four / timing / spec not null when their count is > 0"
POWER_COUNT = "power: n_req must be >= 1 and the request list not null"
MEAS_LIST = "measure: request 0: column out of range"
FOUR_LIST = "fourier: request 0: n_harm outside 1..16"
TIM_LIST = "timing: request 0: targ: n must not be 0"
SPEC_LIST = "spectrum: request 0: log2n outside 3..13"
POWER_LIST = "power: request 0: neg must be 0 or 1"
OUTS = ("meas", "four", "timing", "spec", "power")


@pytest.fixture(scope="module")
def rc():
    from spicey_amd.lib import Handle
    ckt = parseNetlist(RC)
    h = Handle(abi.flatten(ckt))
    yield h, np.ascontiguousarray(abi.source_table(ckt, DT, STEPS), dtype=np.float64)
    h.close()


class L5:
    """One list of a raw call: the records, the count the call states (default: their number) and whether it gets an out array."""

    def __init__(self, reqs, count=None, out=True):
        self.reqs, self.count, self.out = reqs, len(reqs) if count is None else count, out


def _raw(rc, m, f, t, s, p):
    """spicey_run_measure_power on the handle's library with exactly these counts and pointers -> (status, text, arrays, records)."""
    h, src = rc
    from spicey_amd.lib import _p, _reqs_ptr
    outs = {"meas": np.full((1, 2, 8), SENTINEL), "four": np.full((1, 2, 3), SENTINEL), "timing": np.full((1, 2, 8), SENTINEL),
            "spec": np.full((1, 2, 10), SENTINEL), "power": np.full((1, 2, abi.POWER_ROW), SENTINEL), "iters": np.full((1, STEPS + 1), -5, np.int32)}
    args = [h.h, STEPS, DT, _p(src, C.c_double), 0]
    lists = [lst.reqs.copy() for lst in (m, f, t, s, p)]
    for lst, recs, name in zip((m, f, t, s, p), lists, OUTS):
        args += [_reqs_ptr(recs), lst.count, _p(outs[name], C.c_double) if lst.out else None]
        if name in ("four", "spec"):
            args.append(3 if name == "four" else 10)
    status = h.L.spicey_run_measure_power(*args, _p(outs["iters"], C.c_int32))
    # the caller's request records are read, never written
    assert all(a.tobytes() == b.reqs.tobytes() for a, b in zip(lists, (m, f, t, s, p)))
    return status, h.error(), outs


def _refused(rc, text, m, f, t, s, p):
    before = rc[1].copy()
    status, detail, outs = _raw(rc, m, f, t, s, p)
    assert status == abi.ERR_BAD_DESC and detail == text, (status, detail)
    assert all((outs[k] == SENTINEL).all() for k in OUTS) and (outs["iters"] == -5).all() and np.array_equal(rc[1], before), text


def _accepted(rc, reqs, freqs, treqs, sreqs, preqs):
    """Handle.run_measure_power right after a refusal: it works, and exactly the passes that ran took time."""
    h, src = rc
    res = h.run_measure_power(STEPS, DT, src, reqs, freqs, treqs, sreqs, preqs)
    assert res["status"] == abi.OK and res["detail"] == "" and (res["inst_status"] == 0).all() and res["kernel_ms"] > 0
    times = {"measure_ms": h.L.spicey_last_measure_ms(h.h), "fourier_ms": h.L.spicey_last_fourier_ms(h.h), "timing_ms": h.L.spicey_last_timing_ms(h.h),
             "spectrum_ms": h.L.spicey_last_spectrum_ms(h.h), "power_ms": h.L.spicey_last_power_ms(h.h)}
    for k, lst in zip(times, (reqs, freqs, treqs, sreqs, preqs)):
        assert (times[k] > 0) if len(lst) else (times[k] == 0.0), (k, times)
        assert res[k] == times[k]
    assert res["power_ms"] > 0 and res["power"].shape == (1, len(preqs), abi.POWER_ROW)
    # v(in)^2 of the pulse: never negative, the pulse's top at its peak, sum_p = sum_aa = sum_bb, the tail of the row 0
    row = res["power"][0, 0]
    assert row[0] >= 0.0 and row[1] > 0.5 and row[4] == row[7] == row[8] > 1.0 and (row[13:] == 0.0).all()
    return res


def test_run_arguments_and_the_entry_s_own_text(rc):
    ok = (L5(OK_M), L5(OK_F), L5(OK_T), L5(OK_S))
    # the run arguments are judged against `power`, this entry point's own out array, and before anything else
    _refused(rc, RUN_ARGS, L5(OK_M, count=-1), L5(OK_F), L5(OK_T), L5(OK_S), L5(OK_P, out=False))
    _refused(rc, RUN_ARGS, L5(BAD_M), L5(BAD_F), L5(BAD_T), L5(BAD_S), L5(BAD_P, out=False))
    # its own refusals: a negative count or a null out pointer with a positive count in any earlier list — before any list is read
    for k in range(4):
        for fault in (dict(count=-1), dict(out=False)):
            lists = [L5(lst.reqs, **fault) if j == k else lst for j, lst in enumerate(ok)]
            _refused(rc, POWER_ENTRY, *lists, L5(BAD_P))
    _refused(rc, POWER_ENTRY, L5(BAD_M, out=False), L5(BAD_F), L5(BAD_T), L5(BAD_S), L5(BAD_P))
    # its own list: the count
    _refused(rc, POWER_COUNT, *ok, L5(NO_P))
    _refused(rc, POWER_COUNT, *ok, L5(OK_P, count=-1))
    _refused(rc, POWER_COUNT, *ok, L5(OK_P, count=0))
    _accepted(rc, OK_M, OK_F, OK_T, OK_S, OK_P)


def test_the_earliest_faulty_list_wins(rc):
    ref = _accepted(rc, OK_M, OK_F, OK_T, OK_S, OK_P)
    good, bad = (OK_M, OK_F, OK_T, OK_S, OK_P), (BAD_M, BAD_F, BAD_T, BAD_S, BAD_P)
    texts = (MEAS_LIST, FOUR_LIST, TIM_LIST, SPEC_LIST, POWER_LIST)
    # all five, then every pair, then each alone
    _refused(rc, MEAS_LIST, *(L5(b) for b in bad))
    for i in range(5):
        for j in range(i, 5):
            _refused(rc, texts[i], *(L5(bad[k] if k in (i, j) else good[k]) for k in range(5)))
    # empty earlier lists, with null out pointers, are passed over
    none = (L5(NO_M, out=False), L5(NO_F, out=False), L5(NO_T, out=False), L5(NO_S, out=False))
    _refused(rc, POWER_LIST, *none, L5(BAD_P))
    _refused(rc, SPEC_LIST, *none[:3], L5(BAD_S), L5(BAD_P))
    only = _accepted(rc, NO_M, NO_F, NO_T, NO_S, OK_P)
    assert only["meas"].shape == (1, 0, 8) and only["four"].shape == (1, 0, 1) and only["spec"].shape == (1, 0, 1)
    assert np.array_equal(only["power"], ref["power"])
    # the next entry point's call forgets the times of the passes it does not run
    h, src = rc
    res = h.run_measure(STEPS, DT, src, OK_M)
    assert res["status"] == abi.OK and np.array_equal(res["meas"], ref["meas"]) and "power" not in res and "power_ms" not in res
    assert h.L.spicey_last_power_ms(h.h) == 0.0 and h.L.spicey_last_measure_ms(h.h) > 0
