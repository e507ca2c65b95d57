"""Sensitivities and corners of transient measurements on the GPU: spicey_tran_sens_design_device and
spicey_tran_sens_reduce_device bit for bit against the CPU harness (tests/tran_sens_host) and plain numpy, their refusals,
Handle.run_sens / run_levels against a second handle created from the numpy design's values — its run_reduced rows through the
numpy scalars and reduction — over the interpreters, geometries and instance packings, a plain run around them, a singular
perturbed instance, and measureWorstCase against the host route.

Bar: bit identity throughout."""
import numpy as np
import pytest

from conftest import golden_netlist, load_golden
from spicey_amd import abi, measure as M, synth
from spicey_amd import tran_mc as tm
from spicey_amd import tran_sens as ts
from spicey_amd.measure import delay, edge, efficiency, power, rel, rise_time, stats, when
from spicey_amd.netlist import parseNetlist
from tran_sens_host import pytsens as ps

pytestmark = pytest.mark.gpu
OAT = abi.TS_ONE_AT_A_TIME


# (the tests on torch tensors come first: in a process that runs this file alone torch has to open the device before the
# library does, spicey_amd/lib.py load())
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None and a.size else None


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _device_design(R, Cv, Lv, req, act=None, step=None, lvl=None, tol=None):
    import torch

    from spicey_amd import lib
    ni = R.shape[0]
    d_in = [_dev(a) for a in (R, Cv, Lv)]
    d_out = [torch.full(a.shape, float("nan"), dtype=torch.float64, device="cuda") if a.size else None for a in (R, Cv, Lv)]
    need = lib.tran_sens_workspace_bytes(ni, 1, R.shape[1] + Cv.shape[1] + Lv.shape[1], int(req.nA))
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.tran_sens_design_device(ni, R.shape[1], Cv.shape[1], Lv.shape[1], *(_ptr(t) for t in d_in), req, act, step, lvl, tol, *(_ptr(t) for t in d_out),
                                    d_work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return tuple(t.cpu().numpy() if t is not None else np.zeros(a.shape) for t, a in zip(d_out, (R, Cv, Lv)))


def _device_reduce(rows, sc, valid, step, tol):
    import torch

    from spicey_amd import lib
    r = rows[0]
    ni, ns, nA = r.shape[0], len(sc), len(step)
    d_r = _dev(r)
    d_x = torch.full((ni, ns), ps.SENTINEL, dtype=torch.float64, device="cuda")
    d_sens = torch.full((ns, nA, 2), ps.SENTINEL, dtype=torch.float64, device="cuda")
    d_sign = torch.full((ns, nA), ps.SENTINEL_I, dtype=torch.int8, device="cuda")
    d_bound = torch.full((ns, abi.TRAN_SENS_BOUND_ROW), ps.SENTINEL, dtype=torch.float64, device="cuda")
    need = lib.tran_sens_workspace_bytes(ni, ns, 1, nA)
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    triple = [(d_r.data_ptr(), r.shape[1], r.shape[2]), (0, 0, 8), (0, 0, abi.POWER_ROW)]
    torch.cuda.synchronize()
    try:
        lib.tran_sens_reduce_device(ni, triple, sc, valid, step, tol, d_x.data_ptr(), d_sens.data_ptr(), d_sign.data_ptr(), d_bound.data_ptr(), d_work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return d_x.cpu().numpy(), d_sens.cpu().numpy(), d_sign.cpu().numpy(), d_bound.cpu().numpy()


def test_design_device_equals_the_cpu_harness_and_numpy_bit_for_bit():
    for nA in ps.NA:
        shape = (nA // 2 + 1, nA // 3 + 2, nA - nA // 2 - nA // 3 + 1)
        R, Cv, Lv, act, step, lvl, tol = ps.design_inputs(nA, shape, seed=nA)
        for req, kw in ((abi.tran_sens_req(OAT, nA), dict(act=act, step=step)), (abi.tran_sens_req(abi.TS_LEVELS, 0), dict(lvl=lvl, tol=tol))):
            got = _device_design(R, Cv, Lv, req, **kw)
            host = ps.design(R, Cv, Lv, req, **kw)
            ref = ts.design_values(R, Cv, Lv, **kw)
            for a, h, r, what in zip(got, host, ref, "RCL"):
                assert a.shape == h.shape and ps.bits_equal(a, h).all() and ps.bits_equal(a, r).all(), (what, nA, req.mode)


@pytest.mark.parametrize("nA", ps.NA)
def test_reduce_device_equals_the_cpu_harness_and_numpy_bit_for_bit(nA):
    """The shapes and cases of test_tran_sens_host.py: nA around a wave, 1 and 5 scalars, an all-NaN column, an invalid perturbed
    instance, a pair of equal values, ties for the dominant element, a vertex inside the tolerance and one on its edge."""
    for ns in ps.NS:
        for c, case in enumerate(ps.CASES):
            rows, sc, valid, step, tol = ps.case_inputs(case, nA, ns, seed=1000 * nA + 10 * ns + c)
            x, sens, sign, bound = _device_reduce(rows, sc, valid, step, tol)
            hx, hsens, hsign, hbound = ps.reduce(rows, sc, valid, step, tol)
            rx = tm.eval_reference_scalars(sc, rows, valid)
            rsens, rsign, rbound = ts.reduce_reference_tran_sens(rx, valid, step, tol)
            assert ps.bits_equal(x, hx).all() and ps.bits_equal(x, rx).all(), (ns, case)
            assert ps.bits_equal(sens, hsens).all() and ps.bits_equal(sens, rsens).all(), (ns, case)
            assert (sign == hsign).all() and (sign == rsign).all(), (ns, case)
            assert ps.bits_equal(bound, hbound).all() and ps.bits_equal(bound, rbound).all(), (ns, case)


def test_device_refusals_launch_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError
    R, Cv, Lv, act, step, lvl, tol = ps.design_inputs(3, (3, 2, 1), seed=5)
    d_in = [_dev(a) for a in (R, Cv, Lv)]
    outs = [torch.full(a.shape, 7.0, dtype=torch.float64, device="cuda") for a in (R, Cv, Lv)]
    need = lib.tran_sens_workspace_bytes(7, 2, 6, 3)
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def req(mode=OAT, nA=3, **kw):
        q = abi.tran_sens_req(mode, nA)
        for k, val in kw.items():
            setattr(q, k, val)
        return q
    res1 = req()
    res1.reserved[0] = 1
    lv = req(abi.TS_LEVELS, 0)
    bad_t, bad_l = tol.copy(), lvl.copy()
    bad_t[1], bad_l[3, 3] = 1.0, 2
    for q, ni, kw, wb in ((req(struct_bytes=8), 7, {}, need), (res1, 7, {}, need), (req(mode=5), 7, {}, need), (req(nA=2), 7, {}, need), (req(), 0, {}, need),
                          (req(), 7, dict(act=[0, 1, 1]), need), (req(), 7, dict(act=[0, 1, 6]), need), (req(), 7, dict(step=[1e-3, 0.0, 1e-3]), need),
                          (req(), 7, dict(step=[1e-3, np.nan, 1e-3]), need), (req(), 7, dict(step=[1e-3, 1.0, 1e-3]), need), (req(), 7, dict(act=None), need),
                          (req(), 7, {}, 8), (None, 7, {}, need), (lv, 7, dict(tol=bad_t), need), (lv, 7, dict(lvl=bad_l), need), (lv, 7, dict(lvl=None), need),
                          (req(abi.TS_LEVELS, 1), 7, {}, need)):
        args = dict(act=act, step=step, lvl=lvl, tol=tol)
        args.update(kw)
        with pytest.raises(SpiceyNativeError) as e:
            lib.tran_sens_design_device(ni, 3, 2, 1, *(t.data_ptr() for t in d_in), q, args["act"], args["step"], args["lvl"], args["tol"], *(t.data_ptr() for t in outs),
                                        d_work.data_ptr(), wb)
        assert e.value.status == abi.ERR_BAD_DESC and "tran sens: " in str(e.value), str(e.value)
    with pytest.raises(SpiceyNativeError, match="null buffer"):
        lib.tran_sens_design_device(7, 3, 2, 1, *(t.data_ptr() for t in d_in), req(), act, step, None, None, outs[0].data_ptr(), 0, outs[2].data_ptr(), d_work.data_ptr(), need)
    # the reduction
    rows, sc, valid, st, tl = ps.case_inputs("plain", 3, 2, seed=3)
    d_r = _dev(rows[0])
    triple = [(d_r.data_ptr(), 2, 8), (0, 0, 8), (0, 0, abi.POWER_ROW)]
    d_x = torch.full((7, 2), 7.0, dtype=torch.float64, device="cuda")
    d_sens = torch.full((2, 3, 2), 7.0, dtype=torch.float64, device="cuda")
    d_sign = torch.full((2, 3), 7, dtype=torch.int8, device="cuda")
    d_bound = torch.full((2, 8), 7.0, dtype=torch.float64, device="cuda")
    F, K, ADD, GUARD = tm.F, tm.K, tm.ADD, tm.GUARD

    def call(scalars=sc, ni=7, rows_=triple, step_=st, tol_=tl, wb=need, x=None, nA=None):
        lib.tran_sens_reduce_device(ni, rows_, scalars, None, step_, tol_, d_x.data_ptr() if x is None else x, d_sens.data_ptr(), d_sign.data_ptr(), d_bound.data_ptr(),
                                    d_work.data_ptr(), wb, nA=nA)

    bad_sc = sc.copy()
    bad_sc["reserved"][0] = 1
    attempts = [dict(scalars=tm.make_scalars([[F(0, 0, 7)], p], check=False)) for p in ([ADD], [F(0, 0, 0), GUARD], [(9, 0, 0, 0, 0.0)], [F(0, 2, 0)], [F(1, 0, 0)], [K(np.inf)])]
    attempts += [dict(scalars=bad_sc), dict(ni=6), dict(ni=0), dict(nA=2), dict(step_=[1e-3, 1e-3, 1.5]), dict(tol_=[0.1, -0.1, 0.1]), dict(wb=8), dict(x=0),
                 dict(rows_=None), dict(rows_=[(0, 2, 8), triple[1], triple[2]])]
    for kw in attempts:
        with pytest.raises(SpiceyNativeError) as e:
            call(**kw)
        assert e.value.status == abi.ERR_BAD_DESC and "tran sens: " in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == 7.0).all() for o in outs) and (d_work.cpu().numpy() == 0).all()
    assert (d_x.cpu().numpy() == 7.0).all() and (d_sens.cpu().numpy() == 7.0).all() and (d_sign.cpu().numpy() == 7).all() and (d_bound.cpu().numpy() == 7.0).all()
    W = lib.tran_sens_workspace_bytes
    assert W(0, 2, 6, 3) == -1 and W(16385, 2, 6, 3) == -1 and W(7, 0, 6, 3) == -1 and W(7, 2, 0, 3) == -1 and W(7, 2, 6, -1) == -1
    call()  # the good one goes through
    torch.cuda.synchronize()
    assert ps.bits_equal(d_x.cpu().numpy()[:, 0], rows[0][:, 0, 7]).all() and (d_bound.cpu().numpy()[:, 3] == 3).all()


# ---- a run on a handle ---------------------------------------------------------------------------------------------------
def _tol(flat, n_act=None, r=0.02, c=0.05, ind=0.03):
    t = np.concatenate([np.full(flat.nR, r), np.full(flat.nC, c), np.full(flat.nL, ind)])
    if n_act is not None:  # the first n_act of every third element stay active
        keep = np.arange(len(t))[::3][:n_act]
        mask = np.zeros(len(t), bool)
        mask[keep] = True
        t[~mask] = 0.0
    return t


def _case(text, measures):
    ckt = parseNetlist(text)
    tr = ckt.analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    assert steps + 1 <= 101
    plan = M._Plan(ckt, measures, dt, steps)
    names, sc, root = tm.compile_plan(plan, dt)
    return plan.flatten(ckt), steps, dt, abi.source_table(ckt, dt, steps), plan, names, sc


def _circuits():
    boost = golden_netlist(load_golden("boost_probe"))
    return {
        "rc_ladder": (synth.rc_ladder(5, seed=3, tran=".tran 1e-9 6e-8"),
                      {"s": stats("v(n5)"), "tr": rise_time("v(n3)"), "d": delay(edge("v(n2)", rel(0.5)), edge("v(n5)", rel(0.5))), "p": power("R1")}, None),
        "boost_probe": (boost, {"ripple": stats("v(n3)", t_from=0.05), "rise": when("v(n3)", 5.5), "pl": power("RR1"),
                                "eff": efficiency(power("RR1"), power("Vsimulation_voltage_source_0"))}, None),
        "diode_chain": (synth.diode_chain(64, seed=5, tran=".tran 1e-6 4.9e-5"), {"s": stats("v(n64)"), "m": stats("v(n32)", t_from=2e-5)}, 16),
    }


KWS = (dict(), dict(interpreter=1), dict(interpreter=2), dict(interpreter=3), dict(geometry=1), dict(geometry=2), dict(inst_per_wg=1), dict(inst_per_wg=2),
       dict(inst_per_wg=4), dict(force_global=True))


def _rows_of(r, plan):
    return (r["meas"] if len(plan.reqs) else None, r["timing"] if len(plan.treqs) else None, r["power"] if len(plan.preqs) else None)


@pytest.mark.parametrize("name", ("rc_ladder", "boost_probe", "diode_chain"))
def test_run_sens_and_run_levels_equal_a_handle_of_the_designed_values(name):
    """Handle.run_sens and Handle.run_levels against a second handle created from the numpy design's values, run through
    run_reduced with the same options, then the numpy scalars and reduction; a plain run_reduced before and after, from the reset
    state, gives the same bits."""
    from spicey_amd.lib import Handle
    text, measures, n_act = _circuits()[name]
    flat1, steps, dt, src, plan, names, sc = _case(text, measures)
    assert steps <= 50 or name != "diode_chain"
    tol = _tol(flat1, n_act)
    act = np.nonzero(tol > 0)[0].astype(np.int32)
    nA = len(act)
    assert nA == 8 or name != "rc_ladder"
    step = np.where(np.arange(nA) % 2 == 0, 1e-3, 2e-3)
    req = abi.tran_sens_req(OAT, nA)
    flat = flat1.replicate(1 + 2 * nA)
    rng = np.random.default_rng(7)
    n_lv = 9
    lvl = rng.integers(-1, 2, (n_lv, len(tol))).astype(np.int8)
    lvl[0] = 0
    lreq = abi.tran_sens_req(abi.TS_LEVELS, 0)
    flat_l = flat1.replicate(n_lv)
    moved = False
    for kw in KWS:
        h = Handle(flat, **kw)
        before = h.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs)
        h.reset_state()
        res = h.run_sens(steps, dt, src, req, act, step, tol, sc, plan.reqs, plan.treqs, plan.preqs, want_x=True)
        info = h.info()
        h.reset_state()
        after = h.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs)
        h.close()
        assert before["status"] == abi.OK and res["status"] == abi.OK, (kw, res["detail"])
        for key in ("meas", "timing", "power"):
            assert ps.bits_equal(before[key], after[key]).all(), (kw, key)
        for key in ("C_vprev", "L_iprev", "D_vdprev"):
            assert ps.bits_equal(before["state"][key], after["state"][key]).all(), (kw, key)

        def second(designed):
            h2 = Handle(designed, **kw)
            r = h2.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs)
            assert h2.info()["interpreter"] == info["interpreter"] and h2.info()["inst_per_wg"] == info["inst_per_wg"]
            h2.close()
            assert r["status"] == abi.OK
            return r
        ref = second(ps.designed_flat(flat, act, step))
        rx = tm.eval_reference_scalars(sc, _rows_of(ref, plan))
        rsens, rsign, rbound = ts.reduce_reference_tran_sens(rx, None, step, tol[act])
        assert (res["inst_status"] == 0).all() and ps.bits_equal(res["x"], rx).all(), (kw, info)
        assert ps.bits_equal(res["sens"], rsens).all() and (res["sign"] == rsign).all() and ps.bits_equal(res["bound"], rbound).all(), kw
        for key in ("C_vprev", "L_iprev", "D_vdprev"):  # the end state is the designed run's
            assert ps.bits_equal(res["state"][key], ref["state"][key]).all(), (kw, key)
        # instance 0 is the nominal circuit; the designed values did reach the run: some sensitivity is not zero
        assert ps.bits_equal(res["x"][0], tm.eval_reference_scalars(sc, _rows_of(before, plan))[0]).all(), kw
        moved |= bool((res["sign"] != 0).any())
        assert res["sens_ms"] > 0 and res["design_ms"] > 0 and res["kernel_ms"] > 0
        # the levels design on a handle of its own size
        h = Handle(flat_l, **kw)
        lres = h.run_levels(steps, dt, src, lreq, lvl, tol, sc, plan.reqs, plan.treqs, plan.preqs)
        h.reset_state()
        plain = h.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs)
        h.close()
        lref = second(ps.designed_flat(flat_l, lvl=lvl, tol=tol))
        assert lres["status"] == abi.OK and ps.bits_equal(lres["x"], tm.eval_reference_scalars(sc, _rows_of(lref, plan))).all(), kw
        assert ps.bits_equal(lres["x"][0], tm.eval_reference_scalars(sc, _rows_of(plain, plan))[0]).all(), kw
    assert moved


def test_run_sens_refusals_run_nothing():
    from spicey_amd.lib import Handle
    text, measures, _ = _circuits()["boost_probe"]
    flat1, steps, dt, src, plan, names, sc = _case(text, measures)
    tol = _tol(flat1)
    act = np.nonzero(tol > 0)[0].astype(np.int32)
    nA = len(act)
    step = np.full(nA, 1e-3)
    ok = abi.tran_sens_req(OAT, nA)
    h = Handle(flat1.replicate(1 + 2 * nA))
    bad_tol, bad_sc, bad_step, bad_act = tol.copy(), sc.copy(), step.copy(), act.copy()
    bad_tol[1], bad_step[0], bad_act[0] = -0.1, 1.0, len(tol)
    bad_sc[2]["ins"][0]["row"] = 99
    bad_req = abi.tran_sens_req(OAT, nA)
    bad_req.reserved[0] = 1
    four = M.make_four_reqs([(0, 0, -1, 3, 0, steps, 10.0)])
    for kw in (dict(req=bad_req), dict(req=abi.tran_sens_req(OAT, nA - 1)), dict(req=abi.tran_sens_req(abi.TS_LEVELS, 0)), dict(tol=bad_tol), dict(step=bad_step),
               dict(act=bad_act), dict(scalars=bad_sc), dict(freqs=four)):
        args = dict(req=ok, act=act, step=step, tol=tol, scalars=sc, reqs=plan.reqs, treqs=plan.treqs, preqs=plan.preqs)
        args.update(kw)
        res = h.run_sens(steps, dt, src, want_x=True, **args)
        assert res["status"] == abi.ERR_BAD_DESC and "tran sens: " in res["detail"], (kw, res["detail"])
        assert np.isnan(res["sens"]).all() and (res["sign"] == 0).all() and (res["bound"] == 0).all() and np.isnan(res["x"]).all()
    assert "fourier" in h.run_sens(steps, dt, src, ok, act, step, tol, sc, plan.reqs, plan.treqs, plan.preqs, freqs=four)["detail"]
    lvl = np.zeros((1 + 2 * nA, len(tol)), np.int8)
    bad_lvl = lvl.copy()
    bad_lvl[1, 1] = -2
    lreq = abi.tran_sens_req(abi.TS_LEVELS, 0)
    for kw in (dict(req=ok), dict(lvl=bad_lvl), dict(tol=bad_tol), dict(freqs=four)):
        args = dict(req=lreq, lvl=lvl, tol=tol, scalars=sc, reqs=plan.reqs, treqs=plan.treqs, preqs=plan.preqs)
        args.update(kw)
        res = h.run_levels(steps, dt, src, **args)
        assert res["status"] == abi.ERR_BAD_DESC and "tran sens: " in res["detail"] and np.isnan(res["x"]).all(), (kw, res["detail"])
    good = h.run_sens(steps, dt, src, ok, act, step, tol, sc, plan.reqs, plan.treqs, plan.preqs)
    h.close()
    assert good["status"] == abi.OK and (good["bound"][:, 3] <= nA).all() and (good["bound"][:, 3] > 0).any()


# ---- the public interface ---------------------------------------------------------------------------------------------------
RC_PULSE = "V1 in 0 PULSE(0 5 1e-6 1e-7 1e-7 2e-5 4e-5)\nR1 in out 1000\nC1 out 0 2e-9\nR2 out 0 100000\n.tran 4e-7 4e-5\n.end\n"


def _same_result(a, b):
    """Two result dicts equal, NaN-aware and bit for bit, apart from the timings."""
    assert a.keys() == b.keys()
    for k in a:
        if k.endswith("_ms"):
            continue
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and ((a[k] == b[k]) | ((a[k] != a[k]) & (b[k] != b[k]))).all(), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def test_measure_worst_case_exact_order_equals_the_host_route():
    measures = {"tr": rise_time("v(out)", t_to=2e-5), "d": delay(edge("v(in)", 2.5), edge("v(out)", 2.5)), "s": stats("v(out)"), "p": power("R1"),
                "e": efficiency(power("R2"), power("V1"))}
    tol = {"R": 0.05, "C": 0.1}
    ckt = parseNetlist(RC_PULSE)
    dev = ts.measureWorstCase(ckt, measures, tol=tol, full=True, exact_order=True)
    host = ts.measureWorstCase(ckt, measures, tol=tol, full=True, backend=ps.HostTranSensBackend())
    _same_result(dev, host)
    assert dev["sens_ms"] > 0 and dev["corner_ms"] > 0 and dev["n_corners"] >= 2
    # the default engine runs the same analysis
    d = ts.measureSens(ckt, measures, tol=tol)
    a, b = d["scalars"]["s.avg"]["sens"]["R1"], dev["scalars"]["s.avg"]["sens"]["R1"]
    assert abs(a - b) <= 1e-9 * 5 / 2e-3 + 1e-12  # the parity bar 1e-9 on values up to 5 V, over the step 2 h


def test_a_singular_perturbed_instance_stops_its_mate_and_the_call_runs_again():
    """An island grounded through 0.97e15 ohm, stepped by 5 %: instance 3 (R2 up) is singular.  Two instances per workgroup: it
    stops instance 2 (R1 down) with it on a handle, and measureSens repeats the run with one instance per workgroup."""
    from spicey_amd.lib import Handle, HipBackend
    ckt = parseNetlist("V1 a 0 dc 1\nR1 a 0 1k\nR2 x 0 0.97e15\n.tran 1u 5u\n.end\n")
    measures = {"s": stats("v(a)"), "p": power("R1")}
    tol, rel_step = {"R1": 0.02, "R2": 0.05}, {"R2": 0.05}
    tr = ckt.analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    plan = M._Plan(ckt, measures, dt, steps)
    names, sc, root = tm.compile_plan(plan, dt)
    flat = plan.flatten(ckt).replicate(5)
    src = abi.source_table(ckt, dt, steps)
    act, step, t = np.array([0, 1], np.int32), np.array([1e-3, 0.05]), np.array([0.02, 0.05])
    h = Handle(flat, inst_per_wg=2)
    two = h.run_sens(steps, dt, src, abi.tran_sens_req(OAT, 2), act, step, t, sc, plan.reqs, plan.treqs, plan.preqs, want_x=True)
    h.close()
    assert two["status"] == abi.ERR_SINGULAR and two["inst_status"][3] == abi.ERR_SINGULAR and two["inst_status"][2] == -1 and two["inst_status"][0] == 0
    assert (two["bound"][:, 3] == 0).all() and np.isnan(two["sens"]).all() and np.isnan(two["x"][2:4]).all()  # both elements lost an instance
    r = ts.measureSens(ckt, measures, tol=tol, rel_step=rel_step, full=True, backend=HipBackend(inst_per_wg=2))
    host = ts.measureSens(ckt, measures, tol=tol, rel_step=rel_step, full=True, backend=ps.HostTranSensBackend())
    assert r["n_singular"] == 1 and r["n_stopped"] == 0
    for nm in r["names"]:
        s = r["scalars"][nm]
        assert s["sens"]["R2"] is None and s["sens"]["R1"] is not None and s["n_nan"] == 1, nm
        assert abs(s["sens"]["R1"] - host["scalars"][nm]["sens"]["R1"]) <= 1e-9 / 2e-3 * max(abs(s["nominal"] or 0.0), 1e-3) + 1e-12, nm
