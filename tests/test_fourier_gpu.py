"""The harmonics pass on the GPU: spicey_fourier_device on device tensors against the CPU harness (every row bit for bit)
and against reduce_reference_fourier (pyfourier.check_against_reference: the bound of any summation order); its refusals;
Handle.run_measure_fourier in both modes; fourier() through measureTRAN / measureTRANBatch."""
import os
import sys

import numpy as np
import pytest

from batch_variants import variant
from conftest import REPO, bits_equal, farr, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.measure import cross, fourier, make_four_reqs, make_reqs, measureTRAN, measureTRANBatch, stats
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError

for _d in ("measure_host", "fourier_host"):
    sys.path.insert(0, os.path.join(REPO, "tests", _d))
import pyfourier as pf  # noqa: E402
import pymeasure as pm  # noqa: E402

pytestmark = pytest.mark.gpu

N_INST, N_I, DT = 3, 5, 1e-6


def _device_fourier(out_v, out_i, reqs, dt, out_stride=None, work_bytes=None, sentinel=None, with_work=False):
    """spicey_fourier_device on torch tensors; the rows (and on request the workspace) back on the host."""
    import torch

    from spicey_amd import lib
    ni, n_points, n_v = out_v.shape
    d_v = torch.from_numpy(np.ascontiguousarray(out_v)).cuda()
    d_i = torch.from_numpy(np.ascontiguousarray(out_i)).cuda() if out_i is not None else None
    n_req = len(reqs)
    stride = pf.width(reqs) if out_stride is None else out_stride
    d_out = torch.full((ni, max(n_req, 1), max(stride, 1)), float("nan") if sentinel is None else sentinel, dtype=torch.float64, device="cuda")
    need = lib.fourier_workspace_bytes(ni, n_points, reqs)
    nbytes = need if work_bytes is None else work_bytes
    d_work = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.fourier_device(ni, n_points, dt, d_v.data_ptr(), n_v, d_i.data_ptr() if d_i is not None else 0, out_i.shape[2] if out_i is not None else 0,
                           reqs, d_out.data_ptr(), stride, d_work.data_ptr(), nbytes)
    finally:
        torch.cuda.synchronize()
        host, work = d_out.cpu().numpy(), d_work.cpu().numpy()
    return (host[:, :n_req], work) if with_work else host[:, :n_req]


@pytest.mark.parametrize("n_v", [1, 2, 63, 64, 65, 130])
def test_fourier_device_equals_the_cpu_harness_and_the_reference(n_v):
    c = pf.chunk()
    for n_points in (2, c - 1, c, c + 1, 3 * c + 7):
        out_v, out_i = pm.waveforms(N_INST, n_points, n_v, N_I, seed=1000 * n_v + n_points)
        pool = pf.request_pool(n_points, n_v, N_I, 300, DT, seed=n_v + n_points)
        full = _device_fourier(out_v, out_i, pool, DT)
        assert bits_equal(full, pf.run(out_v, out_i, pool, DT)).all(), n_points
        pf.check_against_reference(full, out_v, out_i, pool, DT)
        perm = np.random.default_rng(n_v).permutation(300)[:65]
        sub = _device_fourier(out_v, out_i, pool[perm], DT)
        assert bits_equal(sub, full[:, perm, :sub.shape[2]]).all(), n_points
        one = _device_fourier(out_v, out_i, pool[7:8], DT)
        assert bits_equal(one, full[:, 7:8, :one.shape[2]]).all(), n_points


def test_refusals_return_bad_desc_and_launch_nothing():
    from spicey_amd.lib import SpiceyNativeError, fourier_workspace_bytes
    out_v, out_i = pm.waveforms(2, 10, 3, 2, seed=1)
    f0 = 1.0 / (40.0 * DT)
    ok = (0, 0, -1, 2, 0, -1, f0)
    bad = [(2, 0, -1, 2, 0, -1, f0),  # signal
           (0, 3, -1, 2, 0, -1, f0), (0, -1, -1, 2, 0, -1, f0), (0, 0, 3, 2, 0, -1, f0), (1, 2, -1, 2, 0, -1, f0),  # columns
           (0, 0, -1, 2, -1, 5, f0), (0, 0, -1, 2, 0, 10, f0), (0, 0, -1, 2, 5, 5, f0), (0, 0, -1, 2, 6, 5, f0),  # windows
           (0, 0, -1, 0, 0, -1, f0), (0, 0, -1, 17, 0, -1, f0),  # n_harm
           (0, 0, -1, 2, 0, -1, 0.0), (0, 0, -1, 2, 0, -1, float("inf")), (0, 0, -1, 2, 0, -1, float("nan")),  # f0
           (0, 0, -1, 2, 0, -1, 0.26 / DT)]  # above Nyquist
    need = 256 + 256 + 512 + 2 * 5 * 8
    assert fourier_workspace_bytes(2, 10, make_four_reqs([ok])) == need == pf.workspace_bytes(2, 10, make_four_reqs([ok]))
    # (refused lists have no workspace size: the calls below bring a workspace that would do for the accepted neighbour)
    cases = [(out_i, make_four_reqs([ok, b]), 33, 4096) for b in bad]
    cases.append((None, make_four_reqs([(1, 0, -1, 2, 0, -1, f0)]), 5, 4096))  # signal = 1 without a current buffer
    cases.append((out_i, make_four_reqs([]), 5, 4096))  # n_req = 0
    cases.append((out_i, make_four_reqs([ok]), 4, need))  # a row shorter than 1 + 2 n_harm
    cases.append((out_i, make_four_reqs([ok]), 5, need - 8))  # workspace too small
    for oi, reqs, stride, wb in cases:
        with pytest.raises(SpiceyNativeError) as e:
            _device_fourier(out_v, oi, reqs, DT, out_stride=stride, work_bytes=wb, sentinel=7.0)
        assert e.value.status == abi.ERR_BAD_DESC and "fourier" in str(e.value), str(e.value)
    # nothing ran: the result buffer and the workspace of a refused call keep what they held
    import torch

    from spicey_amd import lib
    d_v = torch.from_numpy(out_v).cuda()
    d_out = torch.full((2, 2, 5), 7.0, dtype=torch.float64, device="cuda")
    d_work = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for reqs, dt, d_o, d_w in ((make_four_reqs([ok, bad[1]]), DT, d_out.data_ptr(), d_work.data_ptr()), (make_four_reqs([ok, bad[10]]), DT, d_out.data_ptr(), d_work.data_ptr()),
                               (make_four_reqs([ok, ok]), -DT, d_out.data_ptr(), d_work.data_ptr()), (make_four_reqs([ok, ok]), DT, 0, d_work.data_ptr()),
                               (make_four_reqs([ok, ok]), DT, d_out.data_ptr(), 0)):  # (the last two: null buffers)
        with pytest.raises(SpiceyNativeError) as e:
            lib.fourier_device(2, 10, dt, d_v.data_ptr(), 3, 0, 0, reqs, d_o, 5, d_w, d_work.numel())
        assert e.value.status == abi.ERR_BAD_DESC and "fourier" in str(e.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 7.0).all() and (d_work.cpu().numpy() == 0).all()
    assert fourier_workspace_bytes(0, 10, make_four_reqs([ok])) == -1 and fourier_workspace_bytes(2, 10, make_four_reqs([bad[6]])) == -1
    # and the accepted neighbour of those calls works, leaving a wider row's tail zero
    got, work = _device_fourier(out_v, out_i, make_four_reqs([ok]), DT, out_stride=7, sentinel=7.0, with_work=True)
    pf.check_against_reference(got[:, :, :5], out_v, out_i, make_four_reqs([ok]), DT)
    assert (got[:, :, 5:].view(np.int64) == 0).all() and work.any()


def _requests_for(n_v, n_i, n_points, f0, n_harm):
    """Harmonics on every column: the whole run, and a window with a reference column."""
    rows, frows = [], []
    for sig, n in ((0, n_v), (1, n_i)):
        for col in range(n):
            frows.append((sig, col, -1, n_harm, 0, -1, f0))
            frows.append((sig, col, (col + 1) % n if n > 1 else -1, 3, n_points // 3, (2 * n_points) // 3, f0))
            rows.append((0, sig, col, -1, 0, -1, 0.0, 0))
    return make_reqs(rows), make_four_reqs(frows)


def test_run_measure_fourier_in_exact_mode_against_the_golden_waveforms():
    from spicey_amd.lib import Handle
    from spicey_amd.measure import _element_names
    g = load_golden("half_bridge")
    ckt = parseNetlist(golden_netlist(g))
    run = g["runs"][0]
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt, probe_filter=True)
    nodes = [int(i) for i in flat.out_nodes] if flat.out_nodes is not None else list(range(1, ckt.nodes.count()))
    gold_v = np.stack([farr(run["V"][ckt.nodes.rev[i]]) for i in nodes], axis=1)[None]
    names = _element_names(ckt)
    assert len(set(names)) == len(names) == flat.n_cur
    gold_i = np.stack([farr(run["I"][nm]) for nm in names], axis=1)[None]
    reqs, freqs = _requests_for(flat.n_out, flat.n_cur, steps + 1, 20e3, 9)  # (the gate drive's 50 us period)
    h = Handle(flat, interpreter=3, diagnostics=1)
    try:
        res = h.run_measure_fourier(steps, dt, abi.source_table(ckt, dt, steps), reqs, freqs)
    finally:
        h.close()
    assert res["status"] == 0 and (res["inst_status"] == 0).all() and res["measure_ms"] > 0 and res["fourier_ms"] > 0 and res["kernel_ms"] > 0
    pf.check_against_reference(res["four"], gold_v, gold_i, freqs, dt)
    assert bits_equal(res["four"], pf.run(gold_v, gold_i, freqs, dt)).all()
    pm.check_against_reference(res["meas"], gold_v, gold_i, reqs, dt)
    st = run["state"]
    assert bits_equal(res["state"]["C_vprev"][0], farr(st["C_vPrev"])).all() and bits_equal(res["state"]["L_iprev"][0], farr(st["L_iPrev"])).all()


def test_run_measure_fourier_in_default_mode_equals_the_reduction_of_run():
    from spicey_amd.lib import Handle
    text = golden_netlist(load_golden("dchain20"))
    ckts = [parseNetlist(variant(text, k)) for k in range(4)]
    dt, steps = abi.computeEffectiveTimeStep(ckts[0].analyses["tran"]["dt"], ckts[0].analyses["tran"]["tstop"])
    flat = abi.stack_instances([abi.flatten(c) for c in ckts])
    tabs = abi.source_tables(ckts, dt, steps)
    assert not np.array_equal(tabs[0], tabs[1])
    kw = dict(inst_per_wg=2, diagnostics=1)
    reqs, freqs = _requests_for(flat.n_out, flat.n_cur, steps + 1, 1.0 / (25 * dt), 9)

    def on_handle(call):
        h = Handle(flat, **kw)
        try:
            assert h.info()["inst_per_wg"] == 2
            return call(h)
        finally:
            h.close()

    ref = on_handle(lambda h: h.run(steps, dt, tabs))
    plain = on_handle(lambda h: h.run_measure(steps, dt, tabs, reqs))
    got = on_handle(lambda h: h.run_measure_fourier(steps, dt, tabs, reqs, freqs))
    assert ref["status"] == 0 and plain["status"] == 0 and got["status"] == 0 and (got["inst_status"] == 0).all()
    assert got["measure_ms"] > 0 and got["fourier_ms"] > 0
    # the rows: the reduction of what run() returned — within the bound of the reference, and the CPU harness's bits
    pf.check_against_reference(got["four"], ref["out_v"], ref["out_i"], freqs, dt)
    assert bits_equal(got["four"], pf.run(ref["out_v"], ref["out_i"], freqs, dt)).all()
    # everything else is run_measure's
    assert bits_equal(got["meas"], plain["meas"]).all() and np.array_equal(got["iters"], plain["iters"]) and np.array_equal(got["iters"], ref["iters"])
    assert got["solves"] == plain["solves"] == ref["solves"] and np.array_equal(got["skip_risk"], plain["skip_risk"])
    for k in ref["state"]:
        assert bits_equal(got["state"][k], plain["state"][k]).all() and bits_equal(got["state"][k], ref["state"][k]).all(), k
    # voltage-only lists: the run records no currents, and the numbers are those of the run that does
    mv, fv = reqs["signal"] == 0, freqs["signal"] == 0
    gv = on_handle(lambda h: h.run_measure_fourier(steps, dt, tabs, reqs[mv], freqs[fv]))
    assert gv["status"] == 0 and bits_equal(gv["meas"], got["meas"][:, mv]).all() and bits_equal(gv["four"], got["four"][:, fv]).all()
    # no measurement list at all, and a shared source table (the other layout of the same entry point)
    g0 = on_handle(lambda h: h.run_measure_fourier(steps, dt, tabs, make_reqs([]), freqs[fv]))
    assert g0["status"] == 0 and g0["meas"].shape == (4, 0, 8) and g0["measure_ms"] == 0.0 and bits_equal(g0["four"], gv["four"]).all()
    ref0 = on_handle(lambda h: h.run(steps, dt, tabs[0]))
    got0 = on_handle(lambda h: h.run_measure_fourier(steps, dt, tabs[0], reqs[mv], freqs[fv]))
    assert ref0["status"] == 0 and got0["status"] == 0
    assert bits_equal(got0["four"], pf.run(ref0["out_v"], None, freqs[fv], dt)).all()
    # a refused harmonics list runs nothing
    badf = freqs[:1].copy()
    badf["n_harm"] = 17
    r = on_handle(lambda h: h.run_measure_fourier(steps, dt, tabs, reqs, badf))
    assert r["status"] == abi.ERR_BAD_DESC and "fourier" in r["detail"]


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
    f0 = 1.0 / (4 * dt)
    reqs = make_reqs([(0, 0, c, -1, 0, -1, 0.0, 0) for c in range(flat.n_out)])
    freqs = make_four_reqs([(sig, c, -1, 1, 1, -1, f0) for sig, n in ((0, flat.n_out), (1, flat.n_cur)) for c in range(n)])
    h = Handle(flat, **kw)
    try:
        got = h.run_measure_fourier(steps, dt, tabs, reqs, freqs)
    finally:
        h.close()
    assert got["status"] == abi.ERR_SINGULAR and got["inst_status"][1] != 0 and np.array_equal(got["inst_status"], ref["inst_status"])
    pf.check_against_reference(got["four"], ref["out_v"], ref["out_i"], freqs, dt, rows=good)
    pm.check_against_reference(got["meas"], ref["out_v"], ref["out_i"], reqs, dt, rows=good)
    # the front end: the error in its slot, that circuit's state left alone, the others as solo calls give them
    m = {"s": stats("v(x)"), "f": fourier("v(a)", f0, harmonics=1, periods=1), "i": fourier(f"i({ckts[0].R[0].name})", f0, harmonics=1)}
    before = ([c.vPrev for c in ckts[1].C], [l.iPrev for l in ckts[1].L])
    out = measureTRANBatch(ckts, m, exact_order=True)
    assert isinstance(out[1], SingularMatrixError) and str(out[1]) == "Singular matrix (real)"
    assert ([c.vPrev for c in ckts[1].C], [l.iPrev for l in ckts[1].L]) == before
    for i in (0, 2, 3):
        assert out[i] == measureTRAN(parseNetlist(texts[i]), m, exact_order=True), i
        assert out[i]["f"]["dc"] == 1.0
    out = measureTRANBatch([parseNetlist(t) for t in texts], m)  # default mode: a stopped workgroup mate runs again
    assert isinstance(out[1], SingularMatrixError) and all(isinstance(out[i], dict) and out[i]["f"]["dc"] == pytest.approx(1.0) for i in (0, 2, 3))


def test_batch_of_16_variants_equals_16_solo_calls_bit_for_bit():
    text = golden_netlist(load_golden("boost_probe"))
    texts = [variant(text, k) for k in range(16)]
    f0 = 200.0  # (five steps of the run's 1 ms grid)
    m = {"peak": stats("v(n3)"), "h": fourier("v(n3)", f0, harmonics=2, periods=4), "il": fourier("i(LL1)", f0, harmonics=1, t_from=0.02),
         "drop": fourier("v(n1,n3)", f0, harmonics=2), "up": cross("v(n3)", 5.0, dir="rise"), "ripple": stats("v(n3)", t_from=0.05)}
    batch = [parseNetlist(t) for t in texts]
    got = measureTRANBatch(batch, m, exact_order=True)
    assert len(got) == 16 and len({repr(g) for g in got}) > 1
    for k, t in enumerate(texts):
        twin = parseNetlist(t)
        solo = measureTRAN(twin, m, exact_order=True)
        assert got[k] == solo, k  # (floats compared by ==: the same bits, no NaN among them)
        assert list(solo) == list(m) and solo["h"]["periods"] == pytest.approx(4.0) and len(solo["h"]["mag"]) == 2
        assert all(v == v for d in solo.values() for v in d.values() if isinstance(v, float))
        assert [c.vPrev for c in batch[k].C] == [c.vPrev for c in twin.C] and [l.iPrev for l in batch[k].L] == [l.iPrev for l in twin.L]
    # the stats and cross entries are what the dict without fourier gives
    plain = measureTRAN(parseNetlist(texts[3]), {k: v for k, v in m.items() if k in ("peak", "up", "ripple")}, exact_order=True)
    assert all(got[3][k] == plain[k] for k in plain)
