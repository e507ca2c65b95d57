"""The waveform measurements on the GPU: spicey_measure_device on device tensors against the CPU harness (bit for bit, all 8
fields) and against reduce_reference (pymeasure.check_against_reference: order-free fields bit for bit, the sums within
the bound of any summation order); its refusals; Handle.run_measure in both modes; measureTRAN / measureTRANBatch."""
import os
import sys

import numpy as np
import pytest

from batch_variants import variant
from conftest import REPO, bits_equal, farr, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.measure import cross, make_reqs, measureTRAN, measureTRANBatch, stats
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError

sys.path.insert(0, os.path.join(REPO, "tests", "measure_host"))
import pymeasure as pm  # noqa: E402

pytestmark = pytest.mark.gpu

N_INST, N_I, DT = 3, 5, 1e-6


def _device_measure(out_v, out_i, reqs, dt, work_bytes=None, sentinel=None):
    """spicey_measure_device on torch tensors; the result back on the host."""
    import torch

    from spicey_amd import lib
    ni, n_points, n_v = out_v.shape
    d_v = torch.from_numpy(np.ascontiguousarray(out_v)).cuda()
    d_i = torch.from_numpy(np.ascontiguousarray(out_i)).cuda() if out_i is not None else None
    n_req = len(reqs)
    d_meas = torch.full((ni, max(n_req, 1), 8), float("nan") if sentinel is None else sentinel, dtype=torch.float64, device="cuda")
    need = lib.measure_workspace_bytes(ni, n_points, max(n_req, 1))
    nbytes = need if work_bytes is None else work_bytes
    d_work = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.measure_device(ni, n_points, dt, d_v.data_ptr(), n_v, d_i.data_ptr() if d_i is not None else 0, out_i.shape[2] if out_i is not None else 0,
                           reqs, d_meas.data_ptr(), d_work.data_ptr(), nbytes)
    finally:
        torch.cuda.synchronize()
        host = d_meas.cpu().numpy()
    return host[:, :n_req]


@pytest.mark.parametrize("n_v", [1, 2, 63, 64, 65, 130])
def test_measure_device_equals_the_cpu_harness_and_the_reference(n_v):
    c = pm.chunk()
    for n_points in (1, 2, c - 1, c, c + 1, 3 * c + 7):
        out_v, out_i = pm.waveforms(N_INST, n_points, n_v, N_I, seed=1000 * n_v + n_points)
        pool = pm.request_pool(n_points, n_v, N_I, 300, seed=n_v + n_points)
        full = _device_measure(out_v, out_i, pool, DT)
        assert bits_equal(full, pm.run(out_v, out_i, pool, DT)).all(), n_points
        pm.check_against_reference(full, out_v, out_i, pool, DT)
        perm = np.random.default_rng(n_v).permutation(300)[:65]
        assert bits_equal(_device_measure(out_v, out_i, pool[perm], DT), full[:, perm]).all(), n_points
        assert bits_equal(_device_measure(out_v, out_i, pool[7:8], DT), full[:, 7:8]).all(), n_points


def test_refusals_return_bad_desc_and_launch_nothing():
    from spicey_amd.lib import SpiceyNativeError, measure_workspace_bytes
    out_v, out_i = pm.waveforms(2, 10, 3, 2, seed=1)
    ok = (0, 0, 0, -1, 0, -1, 0.0, 0)
    bad = [(2, 0, 0, -1, 0, -1, 0.0, 0), (0, 2, 0, -1, 0, -1, 0.0, 0), (1, 0, 0, -1, 0, -1, 0.0, 2),  # kind, signal, dir
           (0, 0, 3, -1, 0, -1, 0.0, 0), (0, 0, -1, -1, 0, -1, 0.0, 0), (0, 0, 0, 3, 0, -1, 0.0, 0), (0, 1, 2, -1, 0, -1, 0.0, 0),  # columns
           (0, 0, 0, -1, -1, 5, 0.0, 0), (0, 0, 0, -1, 0, 10, 0.0, 0), (0, 0, 0, -1, 6, 5, 0.0, 0)]  # windows
    cases = [(out_i, make_reqs([ok, b]), None) for b in bad]
    cases.append((None, make_reqs([(0, 1, 0, -1, 0, -1, 0.0, 0)]), None))  # signal = 1 without a current buffer
    cases.append((out_i, make_reqs([]), None))  # n_req = 0
    cases.append((out_i, make_reqs([ok]), measure_workspace_bytes(2, 10, 1) - 8))  # workspace too small
    for oi, reqs, wb in cases:
        with pytest.raises(SpiceyNativeError) as e:
            _device_measure(out_v, oi, reqs, DT, work_bytes=wb, sentinel=7.0)
        assert e.value.status == abi.ERR_BAD_DESC and "measure" in str(e.value), str(e.value)
    # nothing ran: the result buffer of a refused call keeps what it held
    import torch

    from spicey_amd import lib
    d_v = torch.from_numpy(out_v).cuda()
    d_meas = torch.full((2, 2, 8), 7.0, dtype=torch.float64, device="cuda")
    d_work = torch.zeros(measure_workspace_bytes(2, 10, 2), dtype=torch.uint8, device="cuda")
    with pytest.raises(SpiceyNativeError):
        lib.measure_device(2, 10, DT, d_v.data_ptr(), 3, 0, 0, make_reqs([ok, bad[3]]), d_meas.data_ptr(), d_work.data_ptr(), d_work.numel())
    torch.cuda.synchronize()
    assert (d_meas.cpu().numpy() == 7.0).all() and (d_work.cpu().numpy() == 0).all()
    assert measure_workspace_bytes(0, 10, 1) == -1
    # and the accepted neighbour of those calls works
    got = _device_measure(out_v, out_i, make_reqs([ok]), DT)
    pm.check_against_reference(got, out_v, out_i, make_reqs([ok]), DT)


def _requests_for(n_v, n_i, n_points, ref_v, ref_i):
    """Stats and crossings on every column (the level from the reference waveform of instance 0), whole run and a window."""
    rows = []
    for sig, n, ref in ((0, n_v, ref_v), (1, n_i, ref_i)):
        if ref is None:
            continue
        for col in range(n):
            x = ref[0, :, col]
            level = float((x.min() + x.max()) / 2)
            rows.append((0, sig, col, -1, 0, -1, 0.0, 0))
            rows.append((0, sig, col, (col + 1) % n if n > 1 else -1, n_points // 3, (2 * n_points) // 3, 0.0, 0))
            rows.append((1, sig, col, -1, 0, -1, level, (1, -1, 0)[col % 3]))
    return make_reqs(rows)


@pytest.mark.parametrize("name", ["boost_probe", "diode_switch"])
def test_run_measure_in_exact_mode_against_the_golden_waveforms(name):
    from spicey_amd.lib import Handle
    g = load_golden(name)
    ckt = parseNetlist(golden_netlist(g))
    run = g["runs"][0]
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt, probe_filter=True)
    nodes = [int(i) for i in flat.out_nodes] if flat.out_nodes is not None else list(range(1, ckt.nodes.count()))
    gold_v = np.stack([farr(run["V"][ckt.nodes.rev[i]]) for i in nodes], axis=1)[None]
    from spicey_amd.measure import _element_names
    names = _element_names(ckt)
    assert len(set(names)) == len(names) == flat.n_cur
    gold_i = np.stack([farr(run["I"][nm]) for nm in names], axis=1)[None]
    reqs = _requests_for(flat.n_out, flat.n_cur, steps + 1, gold_v, gold_i)
    h = Handle(flat, interpreter=3, diagnostics=1)
    try:
        res = h.run_measure(steps, dt, abi.source_table(ckt, dt, steps), reqs)
    finally:
        h.close()
    assert res["status"] == 0 and (res["inst_status"] == 0).all() and res["measure_ms"] > 0 and res["kernel_ms"] > 0
    pm.check_against_reference(res["meas"], gold_v, gold_i, reqs, dt)
    st = run["state"]
    assert bits_equal(res["state"]["C_vprev"][0], farr(st["C_vPrev"])).all() and bits_equal(res["state"]["L_iprev"][0], farr(st["L_iPrev"])).all()


@pytest.mark.parametrize("name", ["dchain20", "mesh6"])
def test_run_measure_in_default_mode_equals_the_reduction_of_run(name):
    from spicey_amd.lib import Handle
    text = golden_netlist(load_golden(name))
    ckts = [parseNetlist(variant(text, k)) for k in range(4)]
    dt, steps = abi.computeEffectiveTimeStep(ckts[0].analyses["tran"]["dt"], ckts[0].analyses["tran"]["tstop"])
    flat = abi.stack_instances([abi.flatten(c) for c in ckts])
    tabs = abi.source_tables(ckts, dt, steps)
    assert not np.array_equal(tabs[0], tabs[1])
    kw = dict(inst_per_wg=2, diagnostics=1)
    h = Handle(flat, **kw)
    try:
        assert h.info()["inst_per_wg"] == 2
        ref = h.run(steps, dt, tabs)
    finally:
        h.close()
    assert ref["status"] == 0
    reqs = _requests_for(flat.n_out, flat.n_cur, steps + 1, ref["out_v"], ref["out_i"])
    h = Handle(flat, **kw)
    try:
        got = h.run_measure(steps, dt, tabs, reqs)
        ms = h.L.spicey_last_measure_ms(h.h)
    finally:
        h.close()
    assert got["status"] == 0 and (got["inst_status"] == 0).all() and got["measure_ms"] == ms > 0
    pm.check_against_reference(got["meas"], ref["out_v"], ref["out_i"], reqs, dt)
    assert np.array_equal(got["iters"], ref["iters"]) and got["solves"] == ref["solves"]
    for k in ref["state"]:
        assert bits_equal(got["state"][k], ref["state"][k]).all(), k
    assert np.array_equal(got["skip_risk"], ref["skip_risk"])
    # voltage requests only: the run records no currents (no current buffer is allocated, spicey_run_measure) and the
    # numbers are those of the run that does
    only_v = reqs[reqs["signal"] == 0]
    h = Handle(flat, **kw)
    try:
        gv = h.run_measure(steps, dt, tabs, only_v)
    finally:
        h.close()
    assert gv["status"] == 0 and bits_equal(gv["meas"], got["meas"][:, reqs["signal"] == 0]).all()
    # a shared source table takes the other layout of the same entry point
    both = []
    for call in (lambda h: h.run(steps, dt, tabs[0]), lambda h: h.run_measure(steps, dt, tabs[0], only_v)):
        h = Handle(flat, **kw)
        try:
            both.append(call(h))
        finally:
            h.close()
    ref0, got0 = both
    assert ref0["status"] == 0 and got0["status"] == 0
    pm.check_against_reference(got0["meas"], ref0["out_v"], None, only_v, dt)


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
    reqs = _requests_for(flat.n_out, flat.n_cur, steps + 1, ref["out_v"][good], ref["out_i"][good])
    h = Handle(flat, **kw)
    try:
        got = h.run_measure(steps, dt, tabs, reqs)
    finally:
        h.close()
    assert got["status"] == abi.ERR_SINGULAR and got["inst_status"][1] != 0 and np.array_equal(got["inst_status"], ref["inst_status"])
    pm.check_against_reference(got["meas"], ref["out_v"], ref["out_i"], reqs, dt, rows=good)
    # the front end: the error in its slot, that circuit's state left alone, the others as solo calls give them
    m = {"s": stats("v(x)"), "c": cross("v(x)", 0.0, dir="either"), "i": stats(f"i({ckts[0].R[0].name})")}
    before = ([c.vPrev for c in ckts[1].C], [l.iPrev for l in ckts[1].L])
    out = measureTRANBatch(ckts, m, exact_order=True)
    assert isinstance(out[1], SingularMatrixError) and str(out[1]) == "Singular matrix (real)"
    assert ([c.vPrev for c in ckts[1].C], [l.iPrev for l in ckts[1].L]) == before
    for i in (0, 2, 3):
        assert out[i] == measureTRAN(parseNetlist(texts[i]), m, exact_order=True), i
    out = measureTRANBatch([parseNetlist(t) for t in texts], m)  # default mode: a stopped workgroup mate runs again
    assert isinstance(out[1], SingularMatrixError) and all(isinstance(out[i], dict) and out[i]["s"]["min"] <= out[i]["s"]["max"] for i in (0, 2, 3))


def test_batch_of_16_variants_equals_16_solo_calls_bit_for_bit():
    text = golden_netlist(load_golden("boost_probe"))
    texts = [variant(text, k) for k in range(16)]
    m = {"peak": stats("v(n3)"), "ripple": stats("v(n3)", t_from=0.05), "il": stats("i(LL1)"), "drop": stats("v(n1,n3)"),
         "up": cross("v(n3)", 5.0, dir="rise"), "sw": cross("v(n2)", 2.5, dir="either")}
    batch = [parseNetlist(t) for t in texts]
    got = measureTRANBatch(batch, m, exact_order=True)
    assert len(got) == 16 and len({repr(g) for g in got}) > 1
    for k, t in enumerate(texts):
        twin = parseNetlist(t)
        solo = measureTRAN(twin, m, exact_order=True)
        assert got[k] == solo, k  # (floats compared by ==: the same bits, no NaN among them)
        assert all(v == v for d in solo.values() for v in d.values() if isinstance(v, float))
        assert [c.vPrev for c in batch[k].C] == [c.vPrev for c in twin.C] and [l.iPrev for l in batch[k].L] == [l.iPrev for l in twin.L]
