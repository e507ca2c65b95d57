"""What the values pass and the reduced run by struct refuse on the GPU: every clause of spicey_values_device with its text,
nothing launched and the buffers untouched; spicey_run_reduced's own refusals (struct_bytes, counts, a find without its
timing row) and a refused values list behind accepted others."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO, bits_equal
from spicey_amd import abi
from spicey_amd.measure import make_reqs, make_timing_reqs, make_value_points, make_value_reqs
from spicey_amd.netlist import parseNetlist

sys.path.insert(0, os.path.join(REPO, "tests", "values_host"))
import pyvalues as pv  # noqa: E402

pytestmark = pytest.mark.gpu

DT, SENTINEL = 1e-6, 7.0
TRACE_OK = (0, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, 4)
POINTS_OK = (1, 1, 0, -1, 0, 0, -1, 0, 0, 0, 0, 2, 0)
FIND_OK = (2, 0, 1, -1, 1, 0, -1, 0, 0, 0, 0, 0, 0)
PTS_OK = make_value_points([(0, 0.0), (8, 1.0)])
RC = "* pulse into RC\nV1 in 0 PULSE(0 1 0 1u 1u 20u 40u)\nR1 in out 1k\nC1 out 0 1n\n.tran 1u 100u\n.end\n"


def _ok():
    return make_value_reqs([TRACE_OK, POINTS_OK, FIND_OK])


def _bad(which, field, value, second=None):
    q = _ok()
    q[which][field] = value
    if second:
        q[which][second[0]] = second[1]
    return q


def test_refusals_return_bad_desc_and_launch_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError, values_workspace_bytes
    out_v, out_i = pv.waveforms(2, 10, 3, 2, seed=1)
    timing = np.full((2, 1, 8), -1.0)
    ok = _ok()
    need = values_workspace_bytes(2, 10, ok, 2)
    assert need == 256 + 256 + 256 + 512 == pv.workspace_bytes(2, 10, ok, 2)
    d_v, d_i, d_t = torch.from_numpy(out_v).cuda(), torch.from_numpy(out_i).cuda(), torch.from_numpy(timing).cuda()
    d_out = torch.full((2, 3, 24), SENTINEL, dtype=torch.float64, device="cuda")
    d_work = torch.full((4096,), 5, dtype=torch.uint8, device="cuda")

    def call(reqs=ok, pts=PTS_OK, dt=DT, v=True, i=True, t=True, n_timing=1, out=True, work=True, stride=24, work_bytes=need, n_inst=2, n_points=10):
        lib.values_device(n_inst, n_points, dt, d_v.data_ptr() if v else 0, 3, d_i.data_ptr() if i else 0, 2, reqs, pts, d_t.data_ptr() if t else 0, n_timing,
                          d_out.data_ptr() if out else 0, stride, d_work.data_ptr() if work else 0, work_bytes)

    cases = [("unknown kind", dict(reqs=_bad(0, "kind", 3))), ("unknown signal", dict(reqs=_bad(1, "signal", 2))),
             ("unknown signal of the edge", dict(reqs=_bad(2, "x_signal", -1))),
             ("column out of range", dict(reqs=_bad(0, "col", 3))), ("column out of range", dict(reqs=_bad(1, "col_ref", -2))),
             ("column of the edge out of range", dict(reqs=_bad(2, "x_col", 2))), ("column of the edge out of range", dict(reqs=_bad(2, "x_col_ref", 2))),
             ("without a current buffer", dict(reqs=ok[1:2], i=False)), ("without a current buffer", dict(reqs=ok[2:3], i=False)),
             ("column out of range", dict(reqs=ok[:1], v=False)),
             ("window outside", dict(reqs=_bad(0, "step_from", -1))), ("window outside", dict(reqs=_bad(0, "step_to", 10))),
             ("step_from > step_to", dict(reqs=_bad(0, "step_from", 6, ("step_to", 5)))),
             ("buckets outside", dict(reqs=_bad(0, "buckets", 0))), ("buckets outside", dict(reqs=_bad(0, "buckets", 11))),
             ("buckets outside", dict(reqs=_bad(0, "buckets", abi.TRACE_MAX_BUCKETS + 1))),
             ("point run outside the table", dict(reqs=_bad(1, "first", 1))), ("point run outside the table", dict(reqs=_bad(1, "count", 0))),
             ("point run outside the table", dict(pts=PTS_OK[:1])),
             ("point 1: k outside", dict(pts=make_value_points([(0, 0.0), (9, 0.5)]))), ("point 1: k outside", dict(pts=make_value_points([(0, 0.0), (-1, 0.5)]))),
             ("point 0: f outside", dict(pts=make_value_points([(0, 1.5), (8, 1.0)]))), ("point 0: f outside", dict(pts=make_value_points([(0, -0.5), (8, 1.0)]))),
             ("point 1: f outside", dict(pts=make_value_points([(0, 0.0), (8, float("nan"))]))),
             ("point 1: f outside", dict(pts=make_value_points([(0, 0.0), (8, float("inf"))]))),
             ("need n_points >= 2", dict(reqs=ok[1:2], pts=PTS_OK[:0], n_points=1)), ("need n_points >= 2", dict(reqs=ok[2:3], pts=PTS_OK[:0], n_points=1)),
             ("timing_row outside", dict(reqs=_bad(2, "timing_row", 1))), ("timing_row outside", dict(reqs=_bad(2, "timing_row", -1))),
             ("without timing rows", dict(t=False)),
             ("is shorter than the longest", dict(stride=23)),
             ("workspace of", dict(work_bytes=need - 8)), ("n_req must be >= 1", dict(reqs=ok[:0])),
             ("bad arguments", dict(out=False)), ("bad arguments", dict(work=False)), ("bad arguments", dict(n_inst=0)), ("n_points must be >= 1", dict(n_points=0))]
    cases += [("reserved must be 0", dict(reqs=_bad(k, "reserved", 1))) for k in range(3)]
    cases += [("dt must be finite and > 0", dict(dt=dt)) for dt in (0.0, -1e-6, float("inf"), float("nan"))]
    for text, kw in cases:
        with pytest.raises(SpiceyNativeError) as e:
            call(**kw)
        assert e.value.status == abi.ERR_BAD_DESC and ": values: " in str(e.value) and text in str(e.value), (text, str(e.value))
    # nothing ran: the result buffer and the workspace of a refused call keep what they held
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENTINEL).all() and (d_work.cpu().numpy() == 5).all()
    assert values_workspace_bytes(0, 10, ok, 2) == -1 and values_workspace_bytes(1, 0, ok, 2) == -1 and values_workspace_bytes(1, 10, ok[:0], 2) == -1
    assert values_workspace_bytes(1, 10, ok, 1) == -1
    # and the accepted neighbour of those calls works, without timing rows where no request is a find
    call()
    torch.cuda.synchronize()
    assert bits_equal(d_out.cpu().numpy(), pv.run(out_v, out_i, ok, PTS_OK, DT, timing)).all()
    call(reqs=ok[:2], t=False, n_timing=0)
    torch.cuda.synchronize()
    two = d_out.cpu().numpy().reshape(-1)[:2 * 2 * 24].reshape(2, 2, 24)  # (the rows of a list of two)
    assert bits_equal(two, pv.run(out_v, out_i, ok[:2], PTS_OK, DT, None, out_stride=24)).all()


def test_the_struct_entry_s_refusals():
    import ctypes as C

    from spicey_amd.lib import Handle
    ckt = parseNetlist(RC)
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt)
    src = abi.source_table(ckt, dt, steps)
    reqs = make_reqs([(0, 0, 0, -1, 0, -1, 0.0, 0)])
    treqs = make_timing_reqs([(0, steps, None, (0, 0, -1, 1, 1, abi.TIMING_ABS, 0, 0, 0.5), 0)])
    vreqs = make_value_reqs([(0, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, 8), (2, 1, 0, -1, 0, 0, -1, 0, 0, 0, 0, 0, 0)])
    h = Handle(flat)
    try:
        good = h.run_reduced(steps, dt, src, reqs=reqs, treqs=treqs, vreqs=vreqs)
        assert good["status"] == 0 and good["values"][0, 1, 0] >= 0 and good["values_ms"] > 0
        for kw, text in ((dict(reqs=reqs, struct_bytes=C.sizeof(abi.SpiceyReducedLists) - 8), "reduced: struct_bytes is smaller than sizeof(SpiceyReducedLists)"),
                         (dict(reqs=reqs, struct_bytes=0), "reduced: struct_bytes is smaller than sizeof(SpiceyReducedLists)"),
                         (dict(), "reduced: every list is empty (at least one count must be > 0)"),
                         (dict(reqs=reqs, vreqs=vreqs), "values: request 1: a find request without timing rows"),
                         (dict(treqs=treqs, vreqs=make_value_reqs([(2, 1, 0, -1, 0, 0, -1, 1, 0, 0, 0, 0, 0)])), "values: request 0: timing_row outside [0, n_timing)"),
                         (dict(reqs=reqs, vreqs=make_value_reqs([(0, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, steps + 2)])),
                          "values: request 0: buckets outside 1 .. min(samples of the window, SPICEY_TRACE_MAX_BUCKETS)"),
                         (dict(vreqs=make_value_reqs([(1, 0, 0, -1, 0, 0, -1, 0, 0, 0, 0, 1, 0)])), "values: request 0: point run outside the table (count >= 1)")):
            r = h.run_reduced(steps, dt, src, **kw)
            assert r["status"] == abi.ERR_BAD_DESC and r["detail"] == text, (kw.keys(), r["detail"])
            assert (r["values"] == 0.0).all() and (r["meas"] == 0.0).all()  # (nothing ran, nothing came back)
    finally:
        h.close()
    # a larger struct (a later version's) is read as far as this version knows it, and run_measure gives the same rows
    for call in (lambda g: g.run_reduced(steps, dt, src, reqs=reqs, treqs=treqs, vreqs=vreqs, struct_bytes=C.sizeof(abi.SpiceyReducedLists) + 64),
                 lambda g: g.run_measure(steps, dt, src, reqs)):
        h = Handle(flat)
        try:
            again = call(h)
        finally:
            h.close()
        assert again["status"] == 0 and all(bits_equal(again[k], good[k]).all() for k in ("meas", "timing", "values") if k in again)
