"""The spectrum pass on the GPU: spicey_spectrum_device on device tensors against the CPU harness and against
reduce_reference_spectrum (every row bit for bit), the 128 KiB LDS path at N = 8192, independence from the list, the exact
cases, its refusals; Handle.run_measure_spectrum in both modes; spectrum() / dominant() through measureTRAN /
measureTRANBatch."""
import os
import sys

import numpy as np
import pytest

from batch_variants import variant
from conftest import REPO, bits_equal, farr, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.measure import (dominant, fourier, make_four_reqs, make_reqs, make_spec_reqs, make_timing_reqs, measureTRAN, measureTRANBatch,
                                reduce_reference_spectrum, spectrum, stats, when)
from spicey_amd.netlist import parseNetlist

sys.path.insert(0, os.path.join(REPO, "tests", "spectrum_host"))
import pyspectrum as ps  # noqa: E402

pytestmark = pytest.mark.gpu

N_POINTS = (1 << max(ps.LOG2NS)) + 3


def _device_spectrum(out_v, out_i, reqs, dt=ps.DT, out_stride=None, work_bytes=None, sentinel=None, with_work=False):
    """spicey_spectrum_device on torch tensors; the rows (and on request the workspace) back on the host."""
    import torch

    from spicey_amd import lib
    ni, n_points, n_v = out_v.shape
    d_v = torch.from_numpy(np.ascontiguousarray(out_v)).cuda()
    d_i = torch.from_numpy(np.ascontiguousarray(out_i)).cuda() if out_i is not None else None
    n_req = len(reqs)
    stride = ps.width(reqs) if out_stride is None else out_stride
    d_out = torch.full((ni, max(n_req, 1), max(stride, 1)), float("nan") if sentinel is None else sentinel, dtype=torch.float64, device="cuda")
    need = lib.spectrum_workspace_bytes(ni, n_points, reqs)
    nbytes = need if work_bytes is None else work_bytes
    d_work = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.spectrum_device(ni, n_points, dt, d_v.data_ptr(), n_v, d_i.data_ptr() if d_i is not None else 0, out_i.shape[2] if out_i is not None else 0,
                            reqs, d_out.data_ptr(), stride, d_work.data_ptr(), nbytes)
    finally:
        torch.cuda.synchronize()
        host, work = d_out.cpu().numpy(), d_work.cpu().numpy()
    return (host[:, :n_req], work) if with_work else host[:, :n_req]


@pytest.mark.parametrize("n_v", ps.N_VS)
def test_spectrum_device_equals_the_cpu_harness_and_the_reference(n_v):
    out_v, out_i = ps.waveforms(ps.N_INST, N_POINTS, n_v, ps.N_I, seed=100 + n_v)
    pool = ps.request_pool(N_POINTS, n_v, ps.N_I, seed=n_v)
    full = _device_spectrum(out_v, out_i, pool)
    assert bits_equal(full, ps.run(out_v, out_i, pool)).all()
    assert bits_equal(full, reduce_reference_spectrum(out_v, out_i, pool, ps.DT)).all()
    # independence: a permuted sub-list, a list of one
    perm = np.random.default_rng(n_v).permutation(len(pool))[:17]
    sub = _device_spectrum(out_v, out_i, pool[perm])
    assert bits_equal(sub, full[:, perm, :sub.shape[2]]).all()
    one = _device_spectrum(out_v, out_i, pool[7:8])
    assert bits_equal(one, full[:, 7:8, :one.shape[2]]).all()
    # a run of N + 3 points per N: the last request ends on the run's last sample
    for log2n in ps.LOG2NS:
        N = 1 << log2n
        ov, oi = ps.waveforms(ps.N_INST, N + 3, n_v, ps.N_I, seed=7 * log2n + n_v)
        reqs = ps.request_pool(N + 3, n_v, ps.N_I, seed=log2n, log2ns=(log2n,))
        got = _device_spectrum(ov, oi, reqs)
        assert bits_equal(got, ps.run(ov, oi, reqs)).all() and bits_equal(got, reduce_reference_spectrum(ov, oi, reqs, ps.DT)).all(), log2n


def test_n_8192_runs_in_128_kib_of_lds():
    log2n, N = 13, 8192
    assert ps.lds_bytes(log2n) == 128 * 1024
    out_v, out_i = ps.waveforms(2, N + 3, 2, 1, seed=8192)
    reqs = make_spec_reqs([(0, 0, -1, 0, 3, log2n, 1, 0, N // 2), (0, 1, 0, 1, 0, log2n, 0, 1, N // 2), (0, 1, -1, 0, 0, log2n, 0, 0, N // 2),
                           (0, 0, -1, 1, 3, 4, 1, 1, 8)])
    got = _device_spectrum(out_v, out_i, reqs)
    assert bits_equal(got, ps.run(out_v, out_i, reqs)).all()
    worst = ps.check_against_dft(got, out_v, out_i, reqs, max_log2n=13, bins=64, seed=13)  # (64 seeded bins per request)
    print(f"largest error / bound: {worst:.4f}")
    assert 0.0 < worst <= 1.0


def test_exact_cases_of_the_rectangular_window():
    ni, n_points, log2n = 2, 70, 6
    N, half = 64, 32
    reqs = make_spec_reqs([(0, 0, -1, 0, 3, log2n, 0, 0, half), (0, 0, -1, 1, 3, log2n, 0, 0, half), (0, 0, -1, 1, 3, log2n, 0, 1, half)])
    v = np.zeros((ni, n_points, 1))
    v[0, 3, 0], v[1, 3, 0] = 0.3, -1.7  # an impulse at the window's first sample
    got = _device_spectrum(v, None, reqs)
    for i, x0 in enumerate((0.3, -1.7)):
        assert (got[i, 0, 0:N + 2:2] == x0).all() and (got[i, 0, 1:N + 2:2] == 0.0).all()
        assert got[i, 1, :6].tolist() == [0.0, x0, 0.0, -1.0, x0 * x0, x0 * x0] and got[i, 2, 0] == 1.0
    got = _device_spectrum(np.full((ni, n_points, 1), 0.25), None, reqs)  # the constant 0.25
    assert (got[:, 0, 0] == N / 4).all() and (got[:, 0, 1:N + 2] == 0.0).all() and (got[:, 1, 0] == 0.0).all() and (got[:, 2, 0] == -1.0).all()
    got = _device_spectrum(np.zeros((ni, n_points, 1)), None, reqs)  # all zeros
    assert (got[:, 0] == 0.0).all() and (got[:, 1:, 0] == -1.0).all() and (got[:, 1:, 1:] == 0.0).all()
    v = np.zeros((ni, n_points, 1))
    v[:, 3:3 + N, 0] = 1.0 + np.where(np.arange(N) % 2 == 0, 1.0, -1.0)  # DC and Nyquist tie: the lower bin
    got = _device_spectrum(v, None, reqs)
    assert (got[:, 1, 0] == 0.0).all() and (got[:, 1, 4] == float(N * N)).all() and (got[:, 2, 0] == half).all() and (got[:, 2, 5] == -1.0).all()


def test_refusals_return_bad_desc_and_launch_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError, spectrum_workspace_bytes
    out_v, out_i = ps.waveforms(2, 20, 3, 2, seed=1)
    ok = (0, 0, -1, 0, 0, 4, 1, 0, 8)
    bad = [(2, 0, -1, 0, 0, 4, 1, 0, 8), (0, 0, -1, 2, 0, 4, 1, 0, 8), (0, 0, -1, 0, 0, 4, 2, 0, 8),  # signal, kind, window
           (0, 3, -1, 0, 0, 4, 1, 0, 8), (0, -1, -1, 0, 0, 4, 1, 0, 8), (0, 0, 3, 0, 0, 4, 1, 0, 8), (1, 2, -1, 0, 0, 4, 1, 0, 8),  # columns
           (0, 0, -1, 0, 0, 2, 1, 0, 2), (0, 0, -1, 0, 0, 14, 1, 0, 8),  # log2n
           (0, 0, -1, 0, -1, 4, 1, 0, 8), (0, 0, -1, 0, 5, 4, 1, 0, 8),  # first step
           (0, 0, -1, 0, 0, 4, 1, -1, 8), (0, 0, -1, 0, 0, 4, 1, 0, 9), (0, 0, -1, 0, 0, 4, 1, 5, 4)]  # band
    need = 768
    assert spectrum_workspace_bytes(2, 20, make_spec_reqs([ok])) == need == ps.workspace_bytes(2, 20, make_spec_reqs([ok]))
    cases = [(out_i, make_spec_reqs([ok, b]), 18, 4096, ps.DT) for b in bad]
    cases.append((None, make_spec_reqs([(1, 0, -1, 0, 0, 4, 1, 0, 8)]), 18, 4096, ps.DT))  # signal = 1 without a current buffer
    cases.append((out_i, make_spec_reqs([]), 18, 4096, ps.DT))  # n_req = 0
    cases.append((out_i, make_spec_reqs([ok]), 17, need, ps.DT))  # a row shorter than the band
    cases.append((out_i, make_spec_reqs([ok]), 18, need - 8, ps.DT))  # workspace too small
    cases += [(out_i, make_spec_reqs([ok]), 18, need, dt) for dt in (0.0, -1e-6, float("inf"), float("nan"))]
    for oi, reqs, stride, wb, dt in cases:
        with pytest.raises(SpiceyNativeError) as e:
            _device_spectrum(out_v, oi, reqs, dt=dt, out_stride=stride, work_bytes=wb, sentinel=7.0)
        assert e.value.status == abi.ERR_BAD_DESC and "spectrum" in str(e.value), str(e.value)
    # nothing ran: the result buffer and the workspace of a refused call keep what they held
    d_v = torch.from_numpy(out_v).cuda()
    d_out = torch.full((2, 2, 18), 7.0, dtype=torch.float64, device="cuda")
    d_work = torch.full((4096,), 5, dtype=torch.uint8, device="cuda")
    two = make_spec_reqs([ok, ok])
    for reqs, dt, d_o, d_w in ((make_spec_reqs([ok, bad[3]]), ps.DT, d_out.data_ptr(), d_work.data_ptr()), (make_spec_reqs([ok, bad[8]]), ps.DT, d_out.data_ptr(), d_work.data_ptr()),
                               (two, -ps.DT, d_out.data_ptr(), d_work.data_ptr()), (two, ps.DT, 0, d_work.data_ptr()), (two, ps.DT, d_out.data_ptr(), 0)):  # (the last two: null buffers)
        with pytest.raises(SpiceyNativeError) as e:
            lib.spectrum_device(2, 20, dt, d_v.data_ptr(), 3, 0, 0, reqs, d_o, 18, d_w, d_work.numel())
        assert e.value.status == abi.ERR_BAD_DESC and "spectrum" in str(e.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 7.0).all() and (d_work.cpu().numpy() == 5).all()
    assert spectrum_workspace_bytes(0, 20, make_spec_reqs([ok])) == -1 and spectrum_workspace_bytes(2, 20, make_spec_reqs([bad[10]])) == -1
    # and the accepted neighbour of those calls works, leaving a wider row's tail zero
    got, work = _device_spectrum(out_v, out_i, make_spec_reqs([ok]), out_stride=21, sentinel=7.0, with_work=True)
    assert bits_equal(got[:, :, :18], reduce_reference_spectrum(out_v, out_i, make_spec_reqs([ok]), ps.DT)).all()
    assert (got[:, :, 18:].view(np.int64) == 0).all() and work.any()


def _requests_for(n_v, n_i, n_points):
    """A dominant and a band on every column, from the run's last 32 samples and the 16 before the last one; and a stats
    request per voltage column."""
    srows = []
    for sig, n in ((0, n_v), (1, n_i)):
        for col in range(n):
            srows.append((sig, col, -1, 1, n_points - 32, 5, 1, 1, 16))
            srows.append((sig, col, (col + 1) % n if n > 1 else -1, 0, n_points - 16 - 1, 4, col % 2, 0, 8))
    reqs = make_reqs([(0, 0, c, -1, 0, -1, 0.0, 0) for c in range(n_v)])
    return reqs, make_spec_reqs(srows)


def test_run_measure_spectrum_in_exact_mode_against_the_golden_waveforms():
    from spicey_amd.lib import Handle
    from spicey_amd.measure import _element_names
    g = load_golden("boost_probe")
    ckt = parseNetlist(golden_netlist(g))
    run = g["runs"][0]
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt, probe_filter=True)
    nodes = [int(i) for i in flat.out_nodes] if flat.out_nodes is not None else list(range(1, ckt.nodes.count()))
    gold_v = np.stack([farr(run["V"][ckt.nodes.rev[i]]) for i in nodes], axis=1)[None]
    names = _element_names(ckt)
    assert len(set(names)) == len(names) == flat.n_cur
    gold_i = np.stack([farr(run["I"][nm]) for nm in names], axis=1)[None]
    assert steps + 1 >= 32
    reqs, sreqs = _requests_for(flat.n_out, flat.n_cur, steps + 1)
    h = Handle(flat, interpreter=3, diagnostics=1)
    try:
        res = h.run_measure_spectrum(steps, dt, abi.source_table(ckt, dt, steps), reqs, [], [], sreqs)
    finally:
        h.close()
    assert res["status"] == 0 and (res["inst_status"] == 0).all() and res["measure_ms"] > 0 and res["spectrum_ms"] > 0 and res["kernel_ms"] > 0
    assert res["fourier_ms"] == 0.0 and res["timing_ms"] == 0.0 and res["four"].shape[1] == 0 and res["timing"].shape[1] == 0
    assert bits_equal(res["spec"], reduce_reference_spectrum(gold_v, gold_i, sreqs, dt)).all()
    assert bits_equal(res["spec"], ps.run(gold_v, gold_i, sreqs, dt=dt)).all()
    st = run["state"]
    assert bits_equal(res["state"]["C_vprev"][0], farr(st["C_vPrev"])).all() and bits_equal(res["state"]["L_iprev"][0], farr(st["L_iPrev"])).all()


def test_run_measure_spectrum_in_default_mode_equals_the_reduction_of_run():
    from spicey_amd.lib import Handle
    text = golden_netlist(load_golden("dchain20"))
    ckts = [parseNetlist(variant(text, k)) for k in range(4)]
    dt, steps = abi.computeEffectiveTimeStep(ckts[0].analyses["tran"]["dt"], ckts[0].analyses["tran"]["tstop"])
    flat = abi.stack_instances([abi.flatten(c) for c in ckts])
    tabs = abi.source_tables(ckts, dt, steps)
    assert not np.array_equal(tabs[0], tabs[1]) and steps + 1 >= 32
    kw = dict(inst_per_wg=2, diagnostics=1)
    reqs, sreqs = _requests_for(flat.n_out, flat.n_cur, steps + 1)
    freqs = make_four_reqs([(0, 0, -1, 3, 0, -1, 1.0 / (25 * dt))])
    treqs = make_timing_reqs([(0, steps, None, (0, 0, -1, 1, 1, abi.TIMING_MINMAX, 0, -1, 0.5), 0)])

    def on_handle(call):
        h = Handle(flat, **kw)
        try:
            assert h.info()["inst_per_wg"] == 2
            return call(h)
        finally:
            h.close()

    ref = on_handle(lambda h: h.run(steps, dt, tabs))
    plain = on_handle(lambda h: h.run_measure_timing(steps, dt, tabs, reqs, freqs, treqs))
    got = on_handle(lambda h: h.run_measure_spectrum(steps, dt, tabs, reqs, freqs, treqs, sreqs))  # the earlier lists non-empty
    assert ref["status"] == 0 and plain["status"] == 0 and got["status"] == 0 and (got["inst_status"] == 0).all()
    assert got["measure_ms"] > 0 and got["fourier_ms"] > 0 and got["timing_ms"] > 0 and got["spectrum_ms"] > 0
    # the rows: the reduction of what run() returned, the CPU harness's bits and numpy's
    assert bits_equal(got["spec"], reduce_reference_spectrum(ref["out_v"], ref["out_i"], sreqs, dt)).all()
    assert bits_equal(got["spec"], ps.run(ref["out_v"], ref["out_i"], sreqs, dt=dt)).all()
    # everything else is run_measure_timing's
    for k in ("meas", "four", "timing"):
        assert bits_equal(got[k], plain[k]).all(), k
    assert np.array_equal(got["iters"], plain["iters"]) and np.array_equal(got["iters"], ref["iters"])
    assert got["solves"] == plain["solves"] == ref["solves"] and np.array_equal(got["skip_risk"], plain["skip_risk"])
    for k in ref["state"]:
        assert bits_equal(got["state"][k], plain["state"][k]).all() and bits_equal(got["state"][k], ref["state"][k]).all(), k
    # the earlier lists empty, voltage-only requests: the run records no currents, and the numbers are those of the run that does
    sv = sreqs["signal"] == 0
    g0 = on_handle(lambda h: h.run_measure_spectrum(steps, dt, tabs, [], [], [], sreqs[sv]))
    assert g0["status"] == 0 and g0["meas"].shape == (4, 0, 8) and g0["measure_ms"] == 0.0 and g0["fourier_ms"] == 0.0 and g0["timing_ms"] == 0.0
    assert g0["spectrum_ms"] > 0 and bits_equal(g0["spec"], got["spec"][:, sv, :g0["spec"].shape[2]]).all()
    assert np.array_equal(g0["iters"], ref["iters"])
    # a refused spectrum list runs nothing
    bad = sreqs[:1].copy()
    bad["log2n"] = 14
    r = on_handle(lambda h: h.run_measure_spectrum(steps, dt, tabs, reqs, [], [], bad))
    assert r["status"] == abi.ERR_BAD_DESC and "spectrum" in r["detail"]


def test_batch_of_16_variants_equals_16_solo_calls_bit_for_bit():
    text = golden_netlist(load_golden("boost_probe"))
    texts = [variant(text, k) for k in range(16)]
    m = {"dom": dominant("v(n3)", n=64), "spec": spectrum("v(n3)", n=32, window="rect", t_to=0.05), "il": dominant("i(LL1)", window="rect"),
         "drop": spectrum("v(n1,n3)", n=16, f_to=300.0), "peak": stats("v(n3)"), "h": fourier("v(n3)", 200.0, harmonics=2, periods=4),
         "up": when("v(n3)", 5.0)}
    batch = [parseNetlist(t) for t in texts]
    got = measureTRANBatch(batch, m, exact_order=True)
    assert len(got) == 16 and len({repr(g) for g in got}) > 1
    for k, t in enumerate(texts):
        twin = parseNetlist(t)
        solo = measureTRAN(twin, m, exact_order=True)
        assert got[k] == solo, k  # (floats compared by ==: the same bits, no NaN among them)
        assert list(solo) == list(m) and solo["dom"]["n"] == 64 and len(solo["spec"]["mag"]) == 17 and solo["spec"]["window"] == "rect"
        assert [c.vPrev for c in batch[k].C] == [c.vPrev for c in twin.C] and [l.iPrev for l in batch[k].L] == [l.iPrev for l in twin.L]
    # the other entries are what the dict without these specs gives
    plain = measureTRAN(parseNetlist(texts[3]), {k: v for k, v in m.items() if k in ("peak", "h", "up")}, exact_order=True)
    assert all(got[3][k] == plain[k] for k in plain)
