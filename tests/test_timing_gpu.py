"""The edge-timing pass on the GPU: spicey_timing_device on device tensors against the CPU harness and against
reduce_reference_timing, every field of every row bit for bit (no tolerance anywhere); its refusals;
Handle.run_measure_timing in both modes; when() / delay() / ... through measureTRAN / measureTRANBatch."""
import os
import sys

import numpy as np
import pytest

from batch_variants import variant
from conftest import REPO, bits_equal, farr, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.measure import (cross, delay, edge, fourier, make_four_reqs, make_reqs, make_timing_reqs, measureTRAN, measureTRANBatch,
                                reduce_reference_timing, rel, rise_time, settle, stats, when)
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError

for _d in ("measure_host", "fourier_host", "timing_host"):
    sys.path.insert(0, os.path.join(REPO, "tests", _d))
import pyfourier as pf  # noqa: E402
import pymeasure as pm  # noqa: E402
import pytiming as pt  # noqa: E402

pytestmark = pytest.mark.gpu

N_INST, N_I, DT = 3, 5, 1e-6


def E(col=0, level=0.0, dir=1, n=1, kind=0, base=(0, -1), signal=0, col_ref=-1):
    return (signal, col, col_ref, dir, n, kind, base[0], base[1], level)


def _device_timing(out_v, out_i, reqs, dt, work_bytes=None, sentinel=None, with_work=False):
    """spicey_timing_device on torch tensors; the rows (and on request the workspace) back on the host."""
    import torch

    from spicey_amd import lib
    ni, n_points, n_v = out_v.shape
    d_v = torch.from_numpy(np.ascontiguousarray(out_v)).cuda()
    d_i = torch.from_numpy(np.ascontiguousarray(out_i)).cuda() if out_i is not None else None
    n_req = len(reqs)
    d_out = torch.full((ni, max(n_req, 1), 8), float("nan") if sentinel is None else sentinel, dtype=torch.float64, device="cuda")
    need = lib.timing_workspace_bytes(ni, n_points, reqs)
    nbytes = need if work_bytes is None else work_bytes
    d_work = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.timing_device(ni, n_points, dt, d_v.data_ptr(), n_v, d_i.data_ptr() if d_i is not None else 0, out_i.shape[2] if out_i is not None else 0,
                          reqs, d_out.data_ptr(), d_work.data_ptr(), nbytes)
    finally:
        torch.cuda.synchronize()
        host, work = d_out.cpu().numpy(), d_work.cpu().numpy()
    return (host[:, :n_req], work) if with_work else host[:, :n_req]


@pytest.mark.parametrize("n_v", [1, 2, 63, 64, 65, 130])
def test_timing_device_equals_the_cpu_harness_and_the_reference(n_v):
    from spicey_amd import lib
    c = pt.chunk()
    for n_points in (2, c - 1, c, c + 1, 3 * c + 7):
        out_v, out_i = pm.waveforms(N_INST, n_points, n_v, N_I, seed=1000 * n_v + n_points)
        pool = pt.request_pool(n_points, n_v, N_I, 300, seed=n_v + n_points)
        full = _device_timing(out_v, out_i, pool, DT)
        assert lib.timing_workspace_bytes(N_INST, n_points, pool) == pt.workspace_bytes(N_INST, n_points, pool)
        ref = reduce_reference_timing(out_v, out_i, pool, DT)
        assert bits_equal(full, pt.run(out_v, out_i, pool, DT)).all(), n_points
        assert bits_equal(full, ref).all(), (n_points, np.argwhere(~bits_equal(full, ref))[:4])
        perm = np.random.default_rng(n_v).permutation(300)[:65]
        assert bits_equal(_device_timing(out_v, out_i, pool[perm], DT), full[:, perm]).all(), n_points
        assert bits_equal(_device_timing(out_v, out_i, pool[7:8], DT), full[:, 7:8]).all(), n_points


def test_refusals_return_bad_desc_and_launch_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError, timing_workspace_bytes
    out_v, out_i = pm.waveforms(2, 10, 3, 2, seed=1)
    ok = (0, -1, E(0, 0.5, kind=1), E(1, 0.25), 1)
    nan, inf = float("nan"), float("inf")
    bad_edges = [E(signal=2), E(dir=2), E(kind=3), E(n=0), E(level=nan), E(level=inf, kind=1), E(col=3), E(col=-1), E(col_ref=3), E(signal=1, col=2),
                 E(kind=1, base=(-1, 5)), E(kind=1, base=(0, 10)), E(kind=2, base=(6, 5))]
    bad = [(0, -1, None, e, 0) for e in bad_edges] + [(0, -1, e, E(), 0) for e in bad_edges] + [
        (-1, 5, None, E(), 0), (0, 10, None, E(), 0), (6, 5, None, E(), 0), (5, 5, None, E(), 0), (9, -1, None, E(), 0)]
    need = 256 + 256 + 256 + 512 + 256
    one = make_timing_reqs([ok])
    assert bits_equal(_device_timing(out_v, out_i, one, DT), reduce_reference_timing(out_v, out_i, one, DT)).all()
    assert timing_workspace_bytes(2, 10, one) == need == pt.workspace_bytes(2, 10, one)
    # (refused lists have no workspace size: the calls below bring a workspace that would do for the accepted neighbour)
    cases = [(out_i, make_timing_reqs([ok, b]), 8192) for b in bad]
    no_trig = make_timing_reqs([ok])
    no_trig["has_trig"] = 0  # targ_from_trig without has_trig
    cases.append((out_i, no_trig, 8192))
    cases.append((None, make_timing_reqs([(0, -1, None, E(signal=1), 0)]), 8192))  # signal = 1 without a current buffer
    cases.append((out_i, make_timing_reqs([]), 8192))  # n_req = 0
    cases.append((out_i, one, need - 8))  # workspace too small
    for oi, reqs, wb in cases:
        with pytest.raises(SpiceyNativeError) as e:
            _device_timing(out_v, oi, reqs, DT, work_bytes=wb, sentinel=7.0)
        assert e.value.status == abi.ERR_BAD_DESC and "timing" in str(e.value), str(e.value)
    # nothing ran: the result buffer and the workspace of a refused call keep what they held
    d_v = torch.from_numpy(out_v).cuda()
    d_out = torch.full((2, 2, 8), 7.0, dtype=torch.float64, device="cuda")
    d_work = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    two = make_timing_reqs([ok, ok])
    for reqs, dt, d_o, d_w in ((make_timing_reqs([ok, bad[3]]), DT, d_out.data_ptr(), d_work.data_ptr()), (make_timing_reqs([ok, bad[-1]]), DT, d_out.data_ptr(), d_work.data_ptr()),
                               (two, -DT, d_out.data_ptr(), d_work.data_ptr()), (two, nan, d_out.data_ptr(), d_work.data_ptr()), (two, DT, 0, d_work.data_ptr()),
                               (two, DT, d_out.data_ptr(), 0)):  # (the last two: null buffers)
        with pytest.raises(SpiceyNativeError) as e:
            lib.timing_device(2, 10, dt, d_v.data_ptr(), 3, 0, 0, reqs, d_o, d_w, d_work.numel())
        assert e.value.status == abi.ERR_BAD_DESC and "timing" in str(e.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 7.0).all() and (d_work.cpu().numpy() == 0).all()
    assert timing_workspace_bytes(0, 10, one) == -1 and timing_workspace_bytes(2, 10, make_timing_reqs([ok, bad[-1]])) == -1
    # and the accepted neighbour of those calls works
    got, work = _device_timing(out_v, out_i, one, DT, sentinel=7.0, with_work=True)
    assert bits_equal(got, reduce_reference_timing(out_v, out_i, one, DT)).all() and work.any()


def _requests_for(n_v, n_i, n_points):
    """Edges on every column: the n-th crossings of the column's own mid-level over the whole run, delays between
    neighbouring columns in a window, last crossings of a band around the end value; and stats of every column."""
    rows, trows = [], []
    for sig, n in ((0, n_v), (1, n_i)):
        for col in range(n):
            nb = (col + 1) % n
            trows.append((0, -1, None, E(col, 0.5, dir=0, n=1 + col % 3, kind=1, signal=sig), 0))
            trows.append((n_points // 5, (4 * n_points) // 5, E(col, 0.5, kind=1, signal=sig, base=(0, n_points // 2)),
                          E(nb, 0.5, dir=0, kind=1, signal=sig, col_ref=col if n > 1 and col % 2 else -1), col % 2))
            trows.append((0, -1, None, E(col, 1.02, dir=0, n=-1, kind=2, signal=sig), 0))
            rows.append((0, sig, col, -1, 0, -1, 0.0, 0))
    return make_reqs(rows), make_timing_reqs(trows)


@pytest.mark.parametrize("name", ["boost_probe", "diode_switch", "half_bridge"])
def test_run_measure_timing_in_exact_mode_against_the_golden_waveforms(name):
    from spicey_amd.lib import Handle
    from spicey_amd.measure import _element_names
    g = load_golden(name)
    ckt = parseNetlist(golden_netlist(g))
    run = g["runs"][0]
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt, probe_filter=True)
    nodes = [int(i) for i in flat.out_nodes] if flat.out_nodes is not None else list(range(1, ckt.nodes.count()))
    gold_v = np.stack([farr(run["V"][ckt.nodes.rev[i]]) for i in nodes], axis=1)[None]
    names = _element_names(ckt)
    assert len(set(names)) == len(names) == flat.n_cur
    gold_i = np.stack([farr(run["I"][nm]) for nm in names], axis=1)[None]
    reqs, treqs = _requests_for(flat.n_out, flat.n_cur, steps + 1)
    h = Handle(flat, interpreter=3, diagnostics=1)
    try:
        res = h.run_measure_timing(steps, dt, abi.source_table(ckt, dt, steps), reqs, make_four_reqs([]), treqs)
    finally:
        h.close()
    assert res["status"] == 0 and (res["inst_status"] == 0).all() and res["measure_ms"] > 0 and res["timing_ms"] > 0 and res["kernel_ms"] > 0
    assert res["four"].shape == (1, 0, 1) and res["fourier_ms"] == 0.0
    ref = reduce_reference_timing(gold_v, gold_i, treqs, dt)
    assert bits_equal(res["timing"], ref).all(), np.argwhere(~bits_equal(res["timing"], ref))[:4]
    assert bits_equal(res["timing"], pt.run(gold_v, gold_i, treqs, dt)).all()
    assert (ref[0, :, 3] >= 0).sum() * 4 >= len(treqs) and (ref[0, :, 3] < 0).any()  # (not a comparison of empty rows: found ones and missed ones)
    pm.check_against_reference(res["meas"], gold_v, gold_i, reqs, dt)
    st = run["state"]
    assert bits_equal(res["state"]["C_vprev"][0], farr(st["C_vPrev"])).all() and bits_equal(res["state"]["L_iprev"][0], farr(st["L_iPrev"])).all()


@pytest.mark.parametrize("name", ["dchain20", "mesh6"])
def test_run_measure_timing_in_default_mode_equals_the_reduction_of_run(name):
    from spicey_amd.lib import Handle
    text = golden_netlist(load_golden(name))
    ckts = [parseNetlist(variant(text, k)) for k in range(4)]
    dt, steps = abi.computeEffectiveTimeStep(ckts[0].analyses["tran"]["dt"], ckts[0].analyses["tran"]["tstop"])
    flat = abi.stack_instances([abi.flatten(c) for c in ckts])
    tabs = abi.source_tables(ckts, dt, steps)
    assert not np.array_equal(tabs[0], tabs[1])
    kw = dict(inst_per_wg=2, diagnostics=1)
    reqs, treqs = _requests_for(flat.n_out, flat.n_cur, steps + 1)
    freqs = make_four_reqs([(0, 0, -1, 3, 0, -1, 1.0 / (25 * dt))])

    def on_handle(call):
        h = Handle(flat, **kw)
        try:
            assert h.info()["inst_per_wg"] == 2
            return call(h)
        finally:
            h.close()

    ref = on_handle(lambda h: h.run(steps, dt, tabs))
    got = on_handle(lambda h: h.run_measure_timing(steps, dt, tabs, reqs, freqs, treqs))
    assert ref["status"] == 0 and got["status"] == 0 and (got["inst_status"] == 0).all()
    assert got["measure_ms"] > 0 and got["fourier_ms"] > 0 and got["timing_ms"] > 0
    want = reduce_reference_timing(ref["out_v"], ref["out_i"], treqs, dt)
    assert bits_equal(got["timing"], want).all(), np.argwhere(~bits_equal(got["timing"], want))[:4]
    assert bits_equal(got["timing"], pt.run(ref["out_v"], ref["out_i"], treqs, dt)).all()
    assert (want[:, :, 3] >= 0).any() and (want[:, :, 3] < 0).any()
    # the other passes and the run itself are what they are without the timing pass
    pm.check_against_reference(got["meas"], ref["out_v"], ref["out_i"], reqs, dt)
    pf.check_against_reference(got["four"], ref["out_v"], ref["out_i"], freqs, dt)
    assert np.array_equal(got["iters"], ref["iters"]) and got["solves"] == ref["solves"] and np.array_equal(got["skip_risk"], ref["skip_risk"])
    for k in ref["state"]:
        assert bits_equal(got["state"][k], ref["state"][k]).all(), k
    # voltage-only lists: the run records no currents, and the rows are those of the run that does; no other list at all
    tv = (treqs["targ"]["signal"] == 0) & ((treqs["has_trig"] == 0) | (treqs["trig"]["signal"] == 0))
    gv = on_handle(lambda h: h.run_measure_timing(steps, dt, tabs, make_reqs([]), make_four_reqs([]), treqs[tv]))
    assert gv["status"] == 0 and gv["meas"].shape == (4, 0, 8) and gv["measure_ms"] == 0.0 and bits_equal(gv["timing"], got["timing"][:, tv]).all()
    # a refused timing list runs nothing
    badt = treqs[:1].copy()
    badt["targ"]["n"] = 0
    r = on_handle(lambda h: h.run_measure_timing(steps, dt, tabs, reqs, freqs, badt))
    assert r["status"] == abi.ERR_BAD_DESC and "timing" in r["detail"]


def test_a_singular_instance_in_the_launch():
    from spicey_amd.lib import Handle
    nsb = golden_netlist(load_golden("near_sing_b"))  # an island grounded through 1e16 ohm: singular; through 1k or 2k: not
    texts = [nsb.replace("1e16", "1k"), nsb, nsb.replace("1e16", "2k"), nsb.replace("1e16", "3k")]
    ckts = [parseNetlist(t) for t in texts]
    dt, steps = abi.computeEffectiveTimeStep(ckts[0].analyses["tran"]["dt"], ckts[0].analyses["tran"]["tstop"])
    flat = abi.stack_instances([abi.flatten(c) for c in ckts])
    tabs = abi.source_tables(ckts, dt, steps)
    kw = dict(inst_per_wg=2)  # (instance 0 shares a workgroup with the singular one and is stopped with it)
    h = Handle(flat, **kw)
    try:
        ref = h.run(steps, dt, tabs)  # (per-instance tables: the finished instances' rows come back)
    finally:
        h.close()
    good = [i for i in range(4) if ref["inst_status"][i] == 0]
    assert ref["status"] == abi.ERR_SINGULAR and ref["inst_status"][1] == abi.ERR_SINGULAR and good == [2, 3]
    reqs, treqs = _requests_for(flat.n_out, flat.n_cur, steps + 1)
    h = Handle(flat, **kw)
    try:
        got = h.run_measure_timing(steps, dt, tabs, reqs, make_four_reqs([]), treqs)
    finally:
        h.close()
    assert got["status"] == abi.ERR_SINGULAR and got["inst_status"][1] != 0 and np.array_equal(got["inst_status"], ref["inst_status"])
    want = reduce_reference_timing(ref["out_v"], ref["out_i"], treqs, dt)
    assert bits_equal(got["timing"][good], want[good]).all()
    pm.check_against_reference(got["meas"], ref["out_v"], ref["out_i"], reqs, dt, rows=good)
    # the front end: the error in its slot, that circuit's state left alone, the others as solo calls give them
    m = {"s": stats("v(x)"), "w": when("v(a)", rel(0.5), "either"), "d": delay(trig=edge("v(a)", rel(0.5), "either"), targ=edge("v(x)", rel(0.5, "ends"), "either"))}
    before = ([c.vPrev for c in ckts[1].C], [l.iPrev for l in ckts[1].L])
    out = measureTRANBatch(ckts, m, exact_order=True)
    assert isinstance(out[1], SingularMatrixError) and str(out[1]) == "Singular matrix (real)"
    assert ([c.vPrev for c in ckts[1].C], [l.iPrev for l in ckts[1].L]) == before
    for i in (0, 2, 3):
        assert out[i] == measureTRAN(parseNetlist(texts[i]), m, exact_order=True), i
    out = measureTRANBatch([parseNetlist(t) for t in texts], m)  # default mode: a stopped workgroup mate runs again
    assert isinstance(out[1], SingularMatrixError) and all(isinstance(out[i], dict) and set(out[i]["d"]) >= {"delay", "count_targ"} for i in (0, 2, 3))


def test_batch_of_16_supply_scaled_variants_equals_16_solo_calls_bit_for_bit():
    from spicey_amd.lib import HipBackend
    text = golden_netlist(load_golden("half_bridge"))
    texts = [variant(text, k, values=False) for k in range(16)]  # the supply and the gate amplitude scaled: every variant another level
    m = {"d": delay(trig=edge("v(g1)", rel(0.5)), targ=edge("v(sw)", rel(0.5))), "pp": stats("v(out)"), "r": rise_time("v(out)", 0.1, 0.5, t_to=100e-6),
         "x": cross("v(sw)", 6.0, dir="fall"), "h": fourier("v(out)", 20e3, harmonics=3, periods=2), "s": settle("v(out)", tol=0.05),
         "il": when("i(L1)", rel(0.5), "either"), "pw": delay(trig=edge("v(sw)", rel(0.5)), targ=edge("v(sw)", rel(0.5), "fall"), t_from=40e-6),
         "f2": delay(trig=edge("v(g1)", rel(0.5), "fall", 2), targ=edge("v(sw)", rel(0.5), "fall"))}
    batch = [parseNetlist(t) for t in texts]
    launches = []

    class Counting(HipBackend):
        def run_measure_timing(self, flat, *a, **kw):
            launches.append(flat.n_inst)
            return super().run_measure_timing(flat, *a, **kw)

    got = measureTRANBatch(batch, m, backend=Counting(diagnostics=1, interpreter=3))
    assert launches == [16]  # one launch: the levels are resolved per instance on the device
    assert len(got) == 16 and len({g["d"]["level_targ"] for g in got}) == 16
    for k, t in enumerate(texts):
        twin = parseNetlist(t)
        solo = measureTRAN(twin, m, exact_order=True)
        assert got[k] == solo, k  # (floats compared by ==: the same bits, no NaN among them)
        assert list(solo) == list(m) and solo["d"]["delay"] is not None and solo["pw"]["delay"] > 0 and solo["il"]["t"] is not None
        assert [c.vPrev for c in batch[k].C] == [c.vPrev for c in twin.C] and [l.iPrev for l in batch[k].L] == [l.iPrev for l in twin.L]
    # the other kinds' entries are what the dict without timing gives
    plain = measureTRAN(parseNetlist(texts[3]), {k: v for k, v in m.items() if k in ("pp", "x", "h")}, exact_order=True)
    assert all(got[3][k] == plain[k] for k in plain)
