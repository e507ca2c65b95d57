"""The product pass on the GPU: spicey_power_device on device tensors against the CPU harness (all 16 doubles of every row bit
for bit) and against reduce_reference_power, independence from the list, its refusals; Handle.run_measure_power in both
modes, with and without recorded currents, behind the four other passes, with a singular instance in the launch; power() /
efficiency() through measureTRAN / measureTRANBatch."""
import os
import sys

import numpy as np
import pytest

from batch_variants import variant
from conftest import REPO, bits_equal, farr, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.measure import (_Plan, cross, dominant, efficiency, fourier, make_four_reqs, make_power_reqs, make_reqs, make_spec_reqs, make_timing_reqs,
                                measureTRAN, measureTRANBatch, power, stats, when)
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError

sys.path.insert(0, os.path.join(REPO, "tests", "power_host"))
import pypower as pp  # noqa: E402

pytestmark = pytest.mark.gpu

N_INST, N_I, DT, SENTINEL = 3, 5, 1e-6, 7.0
RC = "* pulse into RC\nV1 in 0 PULSE(0 1 0 1u 1u 20u 40u)\nR1 in out 1k\nC1 out 0 1n\n.tran 1u 100u\n.end\n"


def _device_power(out_v, out_i, reqs, dt=DT, work_bytes=None, sentinel=float("nan")):
    """spicey_power_device on torch tensors; the rows back on the host."""
    import torch

    from spicey_amd import lib
    ni, n_points, n_v = out_v.shape
    d_v = torch.from_numpy(np.ascontiguousarray(out_v)).cuda()
    d_i = torch.from_numpy(np.ascontiguousarray(out_i)).cuda() if out_i is not None else None
    n_req = len(reqs)
    d_out = torch.full((ni, max(n_req, 1), abi.POWER_ROW), sentinel, dtype=torch.float64, device="cuda")
    need = lib.power_workspace_bytes(ni, n_points, max(n_req, 1))
    nbytes = need if work_bytes is None else work_bytes
    d_work = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.power_device(ni, n_points, dt, d_v.data_ptr(), n_v, d_i.data_ptr() if d_i is not None else 0, out_i.shape[2] if out_i is not None else 0,
                         reqs, d_out.data_ptr(), d_work.data_ptr(), nbytes)
    finally:
        torch.cuda.synchronize()
        host = d_out.cpu().numpy()
    return host[:, :n_req]


@pytest.mark.parametrize("n_v", [1, 2, 65, 130])
def test_power_device_equals_the_cpu_harness(n_v):
    c = pp.chunk()
    for n_points in (1, 2, c - 1, c, c + 1, 3 * c + 7):
        out_v, out_i = pp.waveforms(N_INST, n_points, n_v, N_I, seed=1000 * n_v + n_points)
        pool = pp.request_pool(n_points, n_v, N_I, 300, seed=n_v + n_points)
        full = _device_power(out_v, out_i, pool)
        assert bits_equal(full, pp.run(out_v, out_i, pool, DT)).all(), n_points
        if n_points == 3 * c + 7:
            pp.check_against_reference(full, out_v, out_i, pool, DT)
            # independence: a permuted sub-list, lists of one
            perm = np.random.default_rng(n_v).permutation(300)[:65]
            assert bits_equal(_device_power(out_v, out_i, pool[perm]), full[:, perm]).all()
            for k in (0, 7, 150):
                assert bits_equal(_device_power(out_v, out_i, pool[k:k + 1]), full[:, k:k + 1]).all(), k


def test_refusals_return_bad_desc_and_launch_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError, power_workspace_bytes
    out_v, out_i = pp.waveforms(2, 10, 3, 2, seed=1)
    ok = (0, 0, -1, 1, 0, -1, 0, 0, -1)

    def bad(field, value, second=None):
        q = make_power_reqs([ok, ok])
        q[1][field] = value
        if second:
            q[1][second[0]] = second[1]
        return q

    need = power_workspace_bytes(2, 10, 2)
    assert need == 256 + 2 * 1 * 2 * 128 == pp.lib().spicey_power_host_workspace_bytes(2, 10, 2)
    cases = [(out_i, bad("a_signal", 2), need, DT), (out_i, bad("b_signal", -1), need, DT),  # an unknown signal
             (out_i, bad("a_col", 3), need, DT), (out_i, bad("a_col_ref", -2), need, DT), (out_i, bad("b_col", 2), need, DT), (out_i, bad("b_col_ref", 2), need, DT),
             (None, make_power_reqs([ok, ok]), need, DT),  # a current factor without a current buffer
             (out_i, bad("neg", 2), need, DT), (out_i, bad("reserved", 1), need, DT),
             (out_i, bad("step_from", -1), need, DT), (out_i, bad("step_to", 10), need, DT), (out_i, bad("step_from", 6, ("step_to", 5)), need, DT),  # windows
             (out_i, make_power_reqs([ok, ok]), need - 8, DT),  # workspace too small
             (out_i, make_power_reqs([]), need, DT)]  # n_req = 0
    cases += [(out_i, make_power_reqs([ok, ok]), need, dt) for dt in (0.0, -1e-6, float("inf"), float("nan"))]
    for oi, reqs, wb, dt in cases:
        with pytest.raises(SpiceyNativeError) as e:
            _device_power(out_v, oi, reqs, dt=dt, work_bytes=wb, sentinel=SENTINEL)
        assert e.value.status == abi.ERR_BAD_DESC and ": power: " in str(e.value), str(e.value)
    # nothing ran: the result buffer and the workspace of a refused call keep what they held
    d_v, d_i = torch.from_numpy(out_v).cuda(), torch.from_numpy(out_i).cuda()
    d_out = torch.full((2, 2, abi.POWER_ROW), SENTINEL, dtype=torch.float64, device="cuda")
    d_work = torch.full((4096,), 5, dtype=torch.uint8, device="cuda")
    two = make_power_reqs([ok, ok])
    for reqs, dt, d_o, d_w in [(c[1], c[3], d_out.data_ptr(), d_work.data_ptr()) for c in cases if c[0] is not None and c[2] == need and len(c[1])] + \
            [(two, DT, 0, d_work.data_ptr()), (two, DT, d_out.data_ptr(), 0)]:  # (the last two: null buffers)
        with pytest.raises(SpiceyNativeError) as e:
            lib.power_device(2, 10, dt, d_v.data_ptr(), 3, d_i.data_ptr(), 2, reqs, d_o, d_w, need)
        assert e.value.status == abi.ERR_BAD_DESC and ": power: " in str(e.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENTINEL).all() and (d_work.cpu().numpy() == 5).all()
    assert power_workspace_bytes(0, 10, 1) == -1 and power_workspace_bytes(1, 0, 1) == -1 and power_workspace_bytes(1, 10, 0) == -1
    # and the accepted neighbour of those calls works
    got = _device_power(out_v, out_i, two, sentinel=SENTINEL)
    assert bits_equal(got, pp.run(out_v, out_i, two, DT)).all() and (got[:, :, 13:].view(np.int64) == 0).all()


def _requests_for(n_v, n_i, n_points):
    """v i for every current column (with and without a reference node, either sign, the whole run and its middle third),
    v v and i i of neighbouring columns."""
    rows = []
    a, b = n_points // 3, (2 * n_points) // 3
    for c in range(n_i):
        rows.append((0, c % n_v, -1, 1, c, -1, c % 2, 0, -1))
        rows.append((0, c % n_v, (c + 1) % n_v if n_v > 1 else -1, 1, c, -1, (c + 1) % 2, a, b))
        rows.append((1, c, -1, 1, (c + 1) % n_i, (c + 2) % n_i if n_i > 2 else -1, 0, a, n_points - 1))
    for c in range(n_v):
        rows.append((0, c, -1, 0, (c + 1) % n_v, -1, 0, 0, b))
    return make_power_reqs(rows)


@pytest.mark.parametrize("name", ["boost_probe", "diode_switch"])
def test_run_measure_power_in_exact_mode_against_the_golden_waveforms(name):
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
    preqs = _requests_for(flat.n_out, flat.n_cur, steps + 1)
    h = Handle(flat, interpreter=3, diagnostics=1)
    try:
        res = h.run_measure_power(steps, dt, abi.source_table(ckt, dt, steps), [], [], [], [], preqs)
    finally:
        h.close()
    assert res["status"] == 0 and (res["inst_status"] == 0).all() and res["power_ms"] > 0 and res["kernel_ms"] > 0
    assert res["measure_ms"] == res["fourier_ms"] == res["timing_ms"] == res["spectrum_ms"] == 0.0
    assert res["meas"].shape[1] == res["four"].shape[1] == res["timing"].shape[1] == res["spec"].shape[1] == 0 and res["power"].shape == (1, len(preqs), 16)
    assert bits_equal(res["power"], pp.run(gold_v, gold_i, preqs, dt)).all()
    pp.check_against_reference(res["power"], gold_v, gold_i, preqs, dt)
    st = run["state"]
    assert bits_equal(res["state"]["C_vprev"][0], farr(st["C_vPrev"])).all() and bits_equal(res["state"]["L_iprev"][0], farr(st["L_iPrev"])).all()


def test_run_measure_power_in_default_mode_equals_the_reduction_of_run():
    from spicey_amd.lib import Handle
    text = golden_netlist(load_golden("dchain20"))
    ckts = [parseNetlist(variant(text, k)) for k in range(4)]
    dt, steps = abi.computeEffectiveTimeStep(ckts[0].analyses["tran"]["dt"], ckts[0].analyses["tran"]["tstop"])
    flat = abi.stack_instances([abi.flatten(c) for c in ckts])
    tabs = abi.source_tables(ckts, dt, steps)
    assert not np.array_equal(tabs[0], tabs[1]) and steps + 1 >= 32
    kw = dict(inst_per_wg=2, diagnostics=1)
    n_points = steps + 1
    preqs = _requests_for(flat.n_out, flat.n_cur, n_points)
    reqs = make_reqs([(0, 0, c, -1, 0, -1, 0.0, 0) for c in range(flat.n_out)])
    freqs = make_four_reqs([(0, 0, -1, 3, 0, -1, 1.0 / (25 * dt))])
    treqs = make_timing_reqs([(0, steps, None, (0, 0, -1, 1, 1, abi.TIMING_MINMAX, 0, -1, 0.5), 0)])
    sreqs = make_spec_reqs([(0, 0, -1, 1, n_points - 32, 5, 1, 1, 16), (1, 0, -1, 0, n_points - 17, 4, 0, 0, 8)])

    def on_handle(call):
        h = Handle(flat, **kw)
        try:
            assert h.info()["inst_per_wg"] == 2
            return call(h)
        finally:
            h.close()

    ref = on_handle(lambda h: h.run(steps, dt, tabs))
    got = on_handle(lambda h: h.run_measure_power(steps, dt, tabs, [], [], [], [], preqs))
    assert ref["status"] == 0 and got["status"] == 0 and (got["inst_status"] == 0).all() and got["power_ms"] > 0
    # the rows: the reduction of what run() returned, the CPU harness's bits and numpy's
    assert bits_equal(got["power"], pp.run(ref["out_v"], ref["out_i"], preqs, dt)).all()
    pp.check_against_reference(got["power"], ref["out_v"], ref["out_i"], preqs, dt)
    assert np.array_equal(got["iters"], ref["iters"]) and got["solves"] == ref["solves"] and np.array_equal(got["skip_risk"], ref["skip_risk"])
    for k in ref["state"]:
        assert bits_equal(got["state"][k], ref["state"][k]).all(), k
    # only v v products: the run records no currents, and the numbers are those of the run that does
    vv = (preqs["a_signal"] == 0) & (preqs["b_signal"] == 0)
    assert vv.any() and not vv.all()
    gv = on_handle(lambda h: h.run_measure_power(steps, dt, tabs, [], [], [], [], preqs[vv]))
    assert gv["status"] == 0 and bits_equal(gv["power"], got["power"][:, vv]).all() and np.array_equal(gv["iters"], ref["iters"])
    # all five lists: every earlier pass returns exactly the bits it returns alone
    plain = on_handle(lambda h: h.run_measure_spectrum(steps, dt, tabs, reqs, freqs, treqs, sreqs))
    alone = [on_handle(lambda h: h.run_measure(steps, dt, tabs, reqs))["meas"], on_handle(lambda h: h.run_measure_fourier(steps, dt, tabs, [], freqs))["four"],
             on_handle(lambda h: h.run_measure_timing(steps, dt, tabs, [], [], treqs))["timing"],
             on_handle(lambda h: h.run_measure_spectrum(steps, dt, tabs, [], [], [], sreqs))["spec"]]
    five = on_handle(lambda h: h.run_measure_power(steps, dt, tabs, reqs, freqs, treqs, sreqs, preqs))
    assert five["status"] == 0 and all(five[k] > 0 for k in ("measure_ms", "fourier_ms", "timing_ms", "spectrum_ms", "power_ms"))
    for k, one in zip(("meas", "four", "timing", "spec"), alone):
        assert five[k].shape == one.shape == plain[k].shape and bits_equal(five[k], one).all() and bits_equal(five[k], plain[k]).all(), k
    assert bits_equal(five["power"], got["power"]).all()
    # a refused product list runs nothing
    bad = preqs[:1].copy()
    bad["neg"] = 2
    r = on_handle(lambda h: h.run_measure_power(steps, dt, tabs, reqs, [], [], [], bad))
    assert r["status"] == abi.ERR_BAD_DESC and r["detail"] == "power: request 0: neg must be 0 or 1"


def test_currents_are_recorded_only_when_a_product_names_one():
    ckt = parseNetlist(RC)
    vv = {"vv": power("v(in)", "v(out)"), "sq": power("v(in,out)", "v(in,out)")}
    vi = {**vv, "r1": power("R1")}
    assert not _Plan(ckt, vv, 1e-6, 100).need_i and _Plan(ckt, vi, 1e-6, 100).need_i
    a = measureTRAN(parseNetlist(RC), vv)
    b = measureTRAN(parseNetlist(RC), vi)
    assert a["vv"] == b["vv"] and a["sq"] == b["sq"] and list(b) == ["vv", "sq", "r1"]
    # R1 = 1k: v(in,out) i(R1) is (v(in) - v(out))^2 / 1k to the parity bar, and a resistor's power factor is 1
    assert abs(b["r1"]["energy"] - b["sq"]["energy"] / 1e3) <= 1e-9 * b["r1"]["energy"] and abs(b["r1"]["pf"] - 1.0) <= 1e-9
    assert b["r1"]["energy"] > 0 and b["r1"]["min"] >= 0.0


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
    preqs = _requests_for(flat.n_out, flat.n_cur, steps + 1)
    h = Handle(flat, **kw)
    try:
        got = h.run_measure_power(steps, dt, tabs, [], [], [], [], preqs)
    finally:
        h.close()
    assert got["status"] == abi.ERR_SINGULAR and got["inst_status"][1] != 0 and np.array_equal(got["inst_status"], ref["inst_status"])
    assert bits_equal(got["power"][good], pp.run(ref["out_v"][good], ref["out_i"][good], preqs, dt)).all()
    # the front end: the error in its slot, that circuit's state left alone, the others as solo calls give them
    r = ckts[0].R[0].name
    m = {"p": power(r), "e": efficiency(r, ckts[0].V[0].name), "s": stats("v(x)")}
    before = ([c.vPrev for c in ckts[1].C], [l.iPrev for l in ckts[1].L])
    out = measureTRANBatch(ckts, m, exact_order=True)
    assert isinstance(out[1], SingularMatrixError) and str(out[1]) == "Singular matrix (real)"
    assert ([c.vPrev for c in ckts[1].C], [l.iPrev for l in ckts[1].L]) == before
    for i in (0, 2, 3):
        assert out[i] == measureTRAN(parseNetlist(texts[i]), m, exact_order=True), i
    out = measureTRANBatch([parseNetlist(t) for t in texts], m)  # default mode: a stopped workgroup mate runs again
    assert isinstance(out[1], SingularMatrixError) and all(isinstance(out[i], dict) and set(out[i]["p"]) >= {"energy", "avg", "pf"} for i in (0, 2, 3))


def test_batch_of_16_variants_equals_16_solo_calls_bit_for_bit():
    text = golden_netlist(load_golden("boost_probe"))
    texts = [variant(text, k) for k in range(16)]
    src = "Vsimulation_voltage_source_0"
    m = {"sw": power("SM1"), "d": power("DD1", t_from=0.05), "in": power(src), "out": power("v(n3)", "i(RR1)"), "eff": efficiency("RR1", src),
         "late": efficiency(power("v(n3)", "i(RR1)"), src, t_from=0.05), "vv": power("v(n1)", "v(n3)"), "peak": stats("v(n3)"),
         "h": fourier("v(n3)", 200.0, harmonics=2, periods=4), "up": when("v(n3)", 5.0), "dom": dominant("v(n3)", n=64), "x": cross("v(n3)", 5.0)}
    batch = [parseNetlist(t) for t in texts]
    got = measureTRANBatch(batch, m, exact_order=True)
    assert len(got) == 16 and len({repr(g) for g in got}) > 1
    for k, t in enumerate(texts):
        twin = parseNetlist(t)
        solo = measureTRAN(twin, m, exact_order=True)
        assert got[k] == solo, k  # (floats compared by ==: the same bits, no NaN among them)
        assert list(solo) == list(m) and solo["in"]["avg"] < 0 < solo["out"]["avg"] and 0.0 < solo["eff"]["eff"] < 1.0 + 1e-9
        assert solo["eff"]["p_load"] == solo["out"]["avg"] and solo["eff"]["p_source"] == -solo["in"]["avg"]
        assert [c.vPrev for c in batch[k].C] == [c.vPrev for c in twin.C] and [l.iPrev for l in batch[k].L] == [l.iPrev for l in twin.L]
    # the other entries are what the dict without these specs gives
    plain = measureTRAN(parseNetlist(texts[3]), {k: v for k, v in m.items() if k in ("peak", "h", "up", "dom", "x")}, exact_order=True)
    assert all(got[3][k] == plain[k] for k in plain)
