"""Monte Carlo of transient runs on the GPU: spicey_tran_mc_draw_device and spicey_tran_mc_reduce_device bit for bit against the
CPU harness (tests/tran_mc_host) and plain numpy, their refusals, Handle.run_mc against a second handle created from the numpy
draw's values — its run_reduced rows through the numpy scalars and reduction — over the interpreters, geometries and instance
packings, a plain run around a Monte Carlo run, a singular sample, and measureMonteCarlo against the host route.

Bar: bit identity throughout."""
import numpy as np
import pytest

from conftest import golden_netlist, load_golden
from spicey_amd import abi, measure as M, synth
from spicey_amd import tran_mc as tm
from spicey_amd.mc import icdf_table, mc_gains, mc_values
from spicey_amd.measure import delay, edge, efficiency, measureTRANBatch, power, rel, rise_time, stats, when
from spicey_amd.netlist import parseNetlist
from tran_mc_host import pytmc as pt

pytestmark = pytest.mark.gpu


# (the tests on torch tensors come first: in a process that runs this file alone torch has to open the device before the
# library does, spicey_amd/lib.py load())
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None and a.size else None


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _device_draw(R, Cv, Lv, tol, icdf, req):
    import torch

    from spicey_amd import lib
    ni = R.shape[0]
    d_in = [_dev(a) for a in (R, Cv, Lv)]
    d_out = [torch.full(a.shape, float("nan"), dtype=torch.float64, device="cuda") if a.size else None for a in (R, Cv, Lv)]
    need = lib.tran_mc_workspace_bytes(ni, 1, len(tol), req.log2K, 0)
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        lib.tran_mc_draw_device(ni, R.shape[1], Cv.shape[1], Lv.shape[1], *(_ptr(t) for t in d_in), tol, icdf, req, *(_ptr(t) for t in d_out), d_work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return tuple(t.cpu().numpy() if t is not None else np.zeros(a.shape) for t, a in zip(d_out, (R, Cv, Lv)))


def _device_reduce(d_rows, shapes, ni, sc, valid, lo, hi, probs):
    import torch

    from spicey_amd import lib
    ns = len(sc)
    d_x = torch.full((ni, ns), pt.SENTINEL, dtype=torch.float64, device="cuda")
    d_stat = torch.full((ns, abi.TRAN_MC_STAT_HEAD + 2 * len(probs)), pt.SENTINEL, dtype=torch.float64, device="cuda")
    d_sample = torch.full((ni, 2), pt.SENTINEL_I, dtype=torch.int64, device="cuda")
    need = lib.tran_mc_workspace_bytes(ni, ns, 1, 0, len(probs))
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rows = [(_ptr(t), s[1], s[2]) if t is not None else (0, 0, stride) for t, s, stride in zip(d_rows, shapes, abi.MC_PASS_STRIDE)]
    torch.cuda.synchronize()
    try:
        lib.tran_mc_reduce_device(ni, rows, sc, valid, lo, hi, probs, d_x.data_ptr(), d_stat.data_ptr(), d_sample.data_ptr(), d_work.data_ptr(), need)
    finally:
        torch.cuda.synchronize()
    return d_x.cpu().numpy(), d_stat.cpu().numpy(), d_sample.cpu().numpy()


def test_draw_device_equals_the_cpu_harness_and_numpy_bit_for_bit():
    for ni, shape, L in ((1, (1, 0, 0), 0), (2, (3, 2, 1), 1), (65, (64, 1, 65), 10), (65, (0, 63, 2), 3)):
        R, Cv, Lv, tol, icdf = pt.draw_inputs(ni, shape, L, seed=ni + shape[0])
        for keep in (False, True):
            req = abi.tran_mc_req(L, keep, 0x9E3779B97F4A7C15 ^ ni)
            got = _device_draw(R, Cv, Lv, tol, icdf, req)
            host = pt.draw(R, Cv, Lv, tol, icdf, req)
            g = mc_gains(ni, tol, icdf, L, req.seed, keep)
            ref = (R * g[:, :shape[0]], Cv * g[:, shape[0]:shape[0] + shape[1]], Lv * g[:, shape[0] + shape[1]:])
            for a, h, r, what in zip(got, host, ref, "RCL"):
                assert a.shape == h.shape and pt.bits_equal(a, h).all() and pt.bits_equal(a, r).all(), (what, ni, shape, L, keep)


@pytest.mark.parametrize("ni", pt.REDUCE_NI)
def test_reduce_device_equals_the_cpu_harness_and_numpy_bit_for_bit(ni):
    """The shapes and cases of test_tran_mc_host.py: n_inst around a wave and around the powers of two, 1 and 5 scalars, NaNs,
    infinities and zeros of both signs, all-NaN, one valid sample, ties for the extremes, a third of the samples invalid."""
    for ns in pt.REDUCE_NS:
        for c, case in enumerate(pt.CASES):
            rows, sc, valid, lo, hi = pt.case_inputs(case, ni, ns, seed=100 * ni + ns + c)
            x, stat, sample = _device_reduce([_dev(r) for r in rows], [r.shape for r in rows], ni, sc, valid, lo, hi, pt.PROBS)
            hx, hstat, hsample = pt.reduce(rows, sc, valid, lo, hi, pt.PROBS)
            rx = tm.eval_reference_scalars(sc, rows, valid)
            rsample, rstat = tm.reduce_reference_tran_mc(rx, valid, lo, hi, pt.PROBS)
            assert pt.bits_equal(x, hx).all() and pt.bits_equal(x, rx).all(), (ns, case)
            assert (sample == hsample).all() and (sample == rsample).all(), (ns, case)
            assert pt.bits_equal(stat, hstat).all() and pt.bits_equal(stat, rstat).all(), (ns, case)


@pytest.mark.parametrize("ni", (16384, 8193))
def test_reduce_device_at_the_largest_sort(ni):
    """n_pad = 16384: 128 KiB of keys in LDS, 1024 threads, 105 stages; 8193 samples pad the upper half."""
    rows, sc, valid, lo, hi = pt.case_inputs("third_invalid", ni, 2, seed=ni)
    x, stat, sample = _device_reduce([_dev(r) for r in rows], [r.shape for r in rows], ni, sc, valid, lo, hi, pt.PROBS)
    hx, hstat, hsample = pt.reduce(rows, sc, valid, lo, hi, pt.PROBS)
    rsample, rstat = tm.reduce_reference_tran_mc(tm.eval_reference_scalars(sc, rows, valid), valid, lo, hi, pt.PROBS)
    assert pt.bits_equal(x, hx).all() and (sample == hsample).all() and (sample == rsample).all()
    assert pt.bits_equal(stat, hstat).all() and pt.bits_equal(stat, rstat).all()


def test_device_refusals_launch_nothing():
    import torch

    from spicey_amd import lib
    from spicey_amd.lib import SpiceyNativeError
    R, Cv, Lv, tol, icdf = pt.draw_inputs(3, (4, 2, 1), 3, seed=7)
    d_in = [_dev(a) for a in (R, Cv, Lv)]
    outs = [torch.full(a.shape, 7.0, dtype=torch.float64, device="cuda") for a in (R, Cv, Lv)]
    need = lib.tran_mc_workspace_bytes(3, 2, 7, 3, 2)
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    ok = abi.tran_mc_req(3, True, 5)

    def req(**kw):
        q = abi.tran_mc_req(3, True, 5)
        for k, val in kw.items():
            setattr(q, k, val)
        return q
    neg, big, dec = tol.copy(), tol.copy(), icdf.copy()
    neg[3], big[0], dec[4] = -0.01, 1.0 / np.abs(icdf).max(), icdf[3] - 1e-9
    for q, ni, tl, tab, wb in ((req(struct_bytes=8), 3, tol, icdf, need), (req(reserved=1), 3, tol, icdf, need), (req(log2K=13), 3, tol, icdf, need),
                               (ok, 0, tol, icdf, need), (ok, 16385, tol, icdf, need), (ok, 3, neg, icdf, need), (ok, 3, big, icdf, need), (ok, 3, tol, dec, need),
                               (ok, 3, None, icdf, need), (ok, 3, tol, None, need), (ok, 3, tol, icdf, 8), (None, 3, tol, icdf, need)):
        with pytest.raises(SpiceyNativeError) as e:
            lib.tran_mc_draw_device(ni, 4, 2, 1, *(t.data_ptr() for t in d_in), tl, tab, q, *(t.data_ptr() for t in outs), d_work.data_ptr(), wb)
        assert e.value.status == abi.ERR_BAD_DESC and "tran mc: " in str(e.value), str(e.value)
    with pytest.raises(SpiceyNativeError, match="null buffer"):
        lib.tran_mc_draw_device(3, 4, 2, 1, *(t.data_ptr() for t in d_in), tol, icdf, ok, outs[0].data_ptr(), 0, outs[2].data_ptr(), d_work.data_ptr(), need)
    # the reduction
    rows = pt.rows_like(3, 1)
    d_rows = [_dev(r) for r in rows]
    triple = [(t.data_ptr(), r.shape[1], r.shape[2]) for t, r in zip(d_rows, rows)]
    d_x = torch.full((3, 2), 7.0, dtype=torch.float64, device="cuda")
    d_stat = torch.full((2, 12), 7.0, dtype=torch.float64, device="cuda")
    d_sample = torch.full((3, 2), 7, dtype=torch.int64, device="cuda")
    F, K, ADD, GUARD = tm.F, tm.K, tm.ADD, tm.GUARD
    good = [F(0, 0, 0)]
    bad_programs = ([ADD], [K(1.0)] * 5 + [ADD] * 4, [F(0, 0, 0), F(0, 0, 1)], [F(0, 0, 0), GUARD], [(9, 0, 0, 0, 0.0)], [F(3, 0, 0)], [F(0, 3, 0)], [F(2, 0, 16)],
                    [K(np.inf)], [(abi.MCOP_CONST, 0, 0, 1, 1.0)])

    def call(progs=(good, good), ni=3, rows_=triple, probs=(0.1, 0.9), wb=need, x=None, lo=None, mutate=None, n_scalar=None):
        sc = tm.make_scalars(list(progs), check=False)
        if mutate:
            mutate(sc)
        lib.tran_mc_reduce_device(ni, rows_, sc, None, lo, None, probs, d_x.data_ptr() if x is None else x, d_stat.data_ptr(), d_sample.data_ptr(), d_work.data_ptr(), wb,
                                  n_scalar=n_scalar)

    no_timing = [triple[0], (0, 0, 8), triple[2]]
    attempts = [dict(progs=(good, p)) for p in bad_programs] + [dict(progs=(good, [F(1, 0, 0)]), rows_=no_timing), dict(ni=0), dict(ni=16385), dict(probs=(1.5, 0.5)),
                                                                dict(wb=8), dict(x=0), dict(lo=[0.0, np.nan]), dict(rows_=None), dict(n_scalar=0),
                                                                dict(mutate=lambda sc: sc.__setitem__("reserved", 1)), dict(mutate=lambda sc: sc.__setitem__("n_ins", 49)),
                                                                dict(rows_=[(0, 3, 8), triple[1], triple[2]])]
    for kw in attempts:
        with pytest.raises(SpiceyNativeError) as e:
            call(**kw)
        assert e.value.status == abi.ERR_BAD_DESC and "tran mc: " in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == 7.0).all() for o in outs) and (d_work.cpu().numpy() == 0).all()
    assert (d_x.cpu().numpy() == 7.0).all() and (d_stat.cpu().numpy() == 7.0).all() and (d_sample.cpu().numpy() == 7).all()
    W = lib.tran_mc_workspace_bytes
    assert W(0, 2, 7, 3, 2) == -1 and W(16385, 2, 7, 3, 2) == -1 and W(3, 2, 7, 13, 2) == -1 and W(3, 2, 0, 3, 2) == -1 and W(3, 0, 7, 3, 2) == -1
    call()  # the good one goes through
    torch.cuda.synchronize()
    assert pt.bits_equal(d_x.cpu().numpy()[:, 0], rows[0][:, 0, 0]).all()


# ---- a run on a handle ---------------------------------------------------------------------------------------------------
def _tol(flat, r=0.02, c=0.05, ind=0.03):
    t = np.concatenate([np.full(flat.nR, r), np.full(flat.nC, c), np.full(flat.nL, ind)])
    t[::7] = 0.0
    return t


def _case(text, measures, n):
    ckt = parseNetlist(text)
    tr = ckt.analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    assert steps + 1 <= 101 and n <= 65
    plan = M._Plan(ckt, measures, dt, steps)
    names, sc, root = tm.compile_plan(plan, dt)
    return plan.flatten(ckt).replicate(n), steps, dt, abi.source_table(ckt, dt, steps), plan, names, sc


def _circuits():
    boost = golden_netlist(load_golden("boost_probe"))
    return {
        "rc_ladder": (synth.rc_ladder(40, seed=3, tran=".tran 1e-9 9e-8"),
                      {"s": stats("v(n40)"), "tr": rise_time("v(n20)"), "d": delay(edge("v(n2)", rel(0.5)), edge("v(n30)", rel(0.5))), "p": power("R1")}, 65),
        "boost_probe": (boost, {"ripple": stats("v(n3)", t_from=0.05), "rise": when("v(n3)", 5.5), "pl": power("RR1"),
                                "eff": efficiency(power("RR1"), power("Vsimulation_voltage_source_0"))}, 33),
        "diode_chain": (synth.diode_chain(64, seed=5, tran=".tran 1e-6 9e-5"), {"s": stats("v(n64)"), "m": stats("v(n32)", t_from=5e-5)}, 34),
    }


KWS = (dict(), dict(interpreter=1), dict(interpreter=2), dict(interpreter=3), dict(geometry=1), dict(geometry=2), dict(inst_per_wg=1), dict(inst_per_wg=2),
       dict(inst_per_wg=4), dict(force_global=True))


@pytest.mark.parametrize("name", ("rc_ladder", "boost_probe", "diode_chain"))
def test_run_mc_equals_a_handle_of_the_drawn_values(name):
    """Handle.run_mc against a second handle created from the numpy draw's values, run through run_reduced with the same options,
    then the numpy scalars and reduction; a plain run_reduced before and after run_mc, from the reset state, gives the same bits."""
    from spicey_amd.lib import Handle
    text, measures, n = _circuits()[name]
    flat, steps, dt, src, plan, names, sc = _case(text, measures, n)
    icdf, log2K = icdf_table("gauss")
    req = abi.tran_mc_req(log2K, True, 2025)
    tol = _tol(flat)
    lo, hi = np.full(len(names), -np.inf), np.full(len(names), np.inf)
    hi[0] = 1e300
    open_band = False
    for kw in KWS:
        h = Handle(flat, **kw)
        before = h.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs)
        h.reset_state()
        res = h.run_mc(steps, dt, src, req, tol, icdf, sc, lo, hi, pt.PROBS, plan.reqs, plan.treqs, plan.preqs, want_x=True)
        info = h.info()
        h.reset_state()
        after = h.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs)
        h.close()
        assert before["status"] == abi.OK and res["status"] == abi.OK, (kw, res["detail"])
        for key in ("meas", "timing", "power"):
            assert pt.bits_equal(before[key], after[key]).all(), (kw, key)
        for key in ("C_vprev", "L_iprev", "D_vdprev"):
            assert pt.bits_equal(before["state"][key], after["state"][key]).all(), (kw, key)

        def second(drawn):
            h2 = Handle(drawn, **kw)
            r = h2.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs)
            assert h2.info()["interpreter"] == info["interpreter"] and h2.info()["inst_per_wg"] == info["inst_per_wg"]
            h2.close()
            r["rows"] = (r["meas"] if len(plan.reqs) else None, r["timing"] if len(plan.treqs) else None, r["power"] if len(plan.preqs) else None)
            return r
        ref = pt.run_mc_reference(second, flat, steps, dt, src, req, tol, icdf, sc, lo, hi, pt.PROBS, reducer="numpy")
        assert (res["inst_status"] == ref["inst_status"]).all() and (res["inst_status"] == 0).all(), kw
        assert pt.bits_equal(res["x"], ref["x"]).all(), (kw, info)
        assert (res["sample"] == ref["sample"]).all() and pt.bits_equal(res["stat"], ref["stat"]).all(), kw
        for key in ("C_vprev", "L_iprev", "D_vdprev"):  # the end state is the drawn run's
            assert pt.bits_equal(res["state"][key], ref["state"][key]).all(), (kw, key)
        # sample 0 is the nominal circuit; the drawn values did reach the run: some scalar's band is open
        assert pt.bits_equal(res["x"][0], tm.eval_reference_scalars(sc, (before["meas"] if len(plan.reqs) else None, before["timing"] if len(plan.treqs) else None,
                                                                         before["power"] if len(plan.preqs) else None))[0]).all(), kw
        open_band |= bool((res["stat"][:, 8] < res["stat"][:, 8 + 2 * len(pt.PROBS) - 1]).any())
        assert res["mc_ms"] > 0 and res["draw_ms"] > 0 and res["kernel_ms"] > 0
    assert open_band


def test_run_mc_leaves_a_singular_sample_out_and_reports_it():
    from spicey_amd.lib import Handle
    nsb = golden_netlist(load_golden("near_sing_b"))  # an island grounded through 1e16 ohm: singular; through 1k .. 6k: not
    texts = [nsb.replace("1e16", f"{k}k") for k in (1, 2, 3)] + [nsb] + [nsb.replace("1e16", f"{k}k") for k in (4, 5)]
    ckts = [parseNetlist(t) for t in texts]
    dt, steps = abi.computeEffectiveTimeStep(ckts[0].analyses["tran"]["dt"], ckts[0].analyses["tran"]["tstop"])
    plan = M._Plan(ckts[0], {"s": stats("v(x)")}, dt, steps)
    flats = []
    for c in ckts:
        f = abi.flatten(c)
        f.out_nodes = np.ascontiguousarray(plan.out_nodes, dtype=np.int32)
        flats.append(f)
    flat = abi.stack_instances(flats)
    tabs = abi.source_tables(ckts, dt, steps)
    names, sc, root = tm.compile_plan(plan, dt)
    tol = np.zeros(flat.nR + flat.nC + flat.nL)
    req = abi.tran_mc_req(0, True, 1)
    uni = np.array([-1.0, 1.0])
    h = Handle(flat, inst_per_wg=1)
    res = h.run_mc(steps, dt, tabs, req, tol, uni, sc, None, None, pt.PROBS, plan.reqs, want_x=True)
    plain = h.run_reduced(steps, dt, tabs, plan.reqs)
    h.close()
    assert res["status"] == abi.ERR_SINGULAR and res["inst_status"][3] == abi.ERR_SINGULAR and np.count_nonzero(res["inst_status"]) == 1
    assert (res["stat"][:, 0] == 5).all() and (res["sample"][3] == -1).all() and (np.delete(res["sample"], 3, axis=0) == [0, -1]).all()
    valid = (res["inst_status"] == 0).astype(np.uint8)
    x = tm.eval_reference_scalars(sc, (plain["meas"], None, None), valid)
    sample, stat = tm.reduce_reference_tran_mc(x, valid, None, None, pt.PROBS)
    assert pt.bits_equal(res["x"], x).all() and np.isnan(res["x"][3]).all() and pt.bits_equal(res["stat"], stat).all() and (res["sample"] == sample).all()
    # a workgroup mate of the singular sample is stopped with it and leaves the statistics too
    h = Handle(flat, inst_per_wg=2)
    res2 = h.run_mc(steps, dt, tabs, req, tol, uni, sc, None, None, pt.PROBS, plan.reqs)
    h.close()
    assert res2["inst_status"][3] == abi.ERR_SINGULAR and res2["inst_status"][2] == -1 and (res2["stat"][:, 0] == 4).all()


def test_run_mc_refusals_run_nothing():
    from spicey_amd.lib import Handle
    text, measures, _ = _circuits()["boost_probe"]
    flat, steps, dt, src, plan, names, sc = _case(text, measures, 4)
    tol, uni = _tol(flat), np.array([-1.0, 1.0])
    ok = abi.tran_mc_req(0, True, 3)
    h = Handle(flat)
    bad_tol, nan_tab, bad_sc = tol.copy(), uni.copy(), sc.copy()
    bad_tol[1], nan_tab[1] = -0.1, np.nan
    bad_sc[2]["ins"][0]["row"] = 99
    bad_req = abi.tran_mc_req(0, True, 3)
    bad_req.reserved = 1
    four = M.make_four_reqs([(0, 0, -1, 3, 0, steps, 10.0)])
    for kw in (dict(req=bad_req), dict(tol=bad_tol), dict(tol=np.ones_like(tol)), dict(icdf=nan_tab), dict(probs=(0.5, 1.5)), dict(scalars=bad_sc), dict(lo=np.full(len(sc), np.nan)),
               dict(freqs=four), dict(reqs=(), treqs=(), preqs=(), scalars=tm.make_scalars([[tm.K(1.0)]]))):
        args = dict(req=ok, tol=tol, icdf=uni, scalars=sc, lo=None, hi=None, probs=pt.PROBS, reqs=plan.reqs, treqs=plan.treqs, preqs=plan.preqs)
        args.update(kw)
        res = h.run_mc(steps, dt, src, want_x=True, **args)
        assert res["status"] == abi.ERR_BAD_DESC, (kw, res["detail"])
        assert ("tran mc: " in res["detail"]) or ("reduced: " in res["detail"]), res["detail"]
        assert (res["stat"] == 0).all() and (res["sample"] == -1).all() and np.isnan(res["x"]).all()
    assert "fourier" in h.run_mc(steps, dt, src, ok, tol, uni, sc, probs=pt.PROBS, reqs=plan.reqs, treqs=plan.treqs, preqs=plan.preqs, freqs=four)["detail"]
    good = h.run_mc(steps, dt, src, ok, tol, uni, sc, probs=pt.PROBS, reqs=plan.reqs, treqs=plan.treqs, preqs=plan.preqs)
    h.close()
    assert good["status"] == abi.OK and (good["stat"][:, 0] == 4).all()


# ---- the public interface ---------------------------------------------------------------------------------------------------
RC_PULSE = "V1 in 0 PULSE(0 5 1e-6 1e-7 1e-7 2e-5 4e-5)\nR1 in out 1000\nC1 out 0 2e-9\nR2 out 0 100000\n.tran 4e-7 4e-5\n.end\n"


def test_measure_monte_carlo_exact_order_equals_the_host_route_bit_for_bit():
    measures = {"tr": rise_time("v(out)", t_to=2e-5), "d": delay(edge("v(in)", 2.5), edge("v(out)", 2.5)), "s": stats("v(out)"), "p": power("R1"),
                "e": efficiency(power("R2"), power("V1"))}
    tol, n, seed, probs = {"R": 0.05, "C": 0.1}, 24, 4, (0.0, 0.25, 0.5, 1.0)
    limits = {"s.pp": (None, 4.952), "tr.time": (0, 4.75e-6)}
    ckt = parseNetlist(RC_PULSE)
    r = tm.measureMonteCarlo(ckt, measures, tol=tol, n=n, seed=seed, quantiles=probs, limits=limits, full=True, exact_order=True)
    variants = []
    for s in range(n):
        c = parseNetlist(RC_PULSE)
        vals = mc_values(c, tol, seed, s)
        for e in c.R:
            e.R = vals[e.name]
        for e in c.C:
            e.C = vals[e.name]
        variants.append(c)
    batch = measureTRANBatch(variants, measures, exact_order=True)
    names = r["names"]
    want = np.array([[np.nan if b[nm.split(".")[0]][nm.split(".")[1]] is None else float(b[nm.split(".")[0]][nm.split(".")[1]]) for nm in names] for b in batch])
    assert pt.bits_equal(r["x"], want).all()
    tr = ckt.analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    _, _, root = tm.compile_plan(M._Plan(ckt, measures, dt, steps), dt)
    lo, hi = tm._limit_arrays(limits, names, root)
    plain = np.nonzero(~root)[0]
    sample, stat = tm.reduce_reference_tran_mc(want[:, plain], None, lo[plain], hi[plain], probs)
    for k, j in enumerate(plain):
        s = r["scalars"][names[j]]
        assert s["n_valid"] == n and s["n_nan"] == n - int(stat[k, 1]) and s["yield"] == 1.0 - stat[k, 2] / n
        assert s["worst_low"] == int(stat[k, 5]) and s["worst_high"] == int(stat[k, 6])
        for q, p in enumerate(probs):
            assert pt.bits_equal(np.array([s["quantiles"][p]]), np.array([tm._interp(stat[k, 8 + 2 * q], stat[k, 9 + 2 * q], p, int(stat[k, 1]), False)])).all()
        assert pt.bits_equal(np.array([s["mean"]]), np.array([stat[k, 3] / stat[k, 1]])).all()
    assert 0 < len(r["failing"]) < n and r["n_singular"] == 0 and r["n_stopped"] == 0
    # the default engine runs the same analysis
    d = tm.measureMonteCarlo(ckt, measures, tol=tol, n=n, seed=seed, quantiles=probs, limits=limits)
    assert d["n_valid"] == n and abs(d["scalars"]["s.pp"]["quantiles"][0.5] - r["scalars"]["s.pp"]["quantiles"][0.5]) <= 1e-9 * 5 + 1e-12


def test_drawn_samples_that_turn_singular_leave_the_statistics_and_stopped_mates_run_again():
    """An island grounded through 0.97e15 ohm with 5 % on that resistor: the samples drawn above 1e15 ohm (1 / R below EPS) are
    singular.  Two samples per workgroup: a singular one stops its mate, so measureMonteCarlo runs the draw again with one sample
    per workgroup.  On a handle the valid samples equal a handle created from the numpy draw's values, bit for bit."""
    from spicey_amd.lib import Handle, HipBackend
    text = "V1 a 0 dc 1\nR1 a 0 1k\nR2 x 0 0.97e15\n.tran 1u 5u\n.end\n"
    measures = {"s": stats("v(a)"), "p": power("R1")}
    tol, n, seed = {"R1": 0.02, "R2": 0.05}, 24, 12
    ckt = parseNetlist(text)
    vals = [mc_values(ckt, tol, seed, s, dist="uniform") for s in range(n)]
    r2 = np.array([v["R2"] for v in vals])
    assert (np.abs(r2 - 1e15) > 1e-6 * 1e15).all()  # (no sample sits on the threshold)
    sing = r2 > 1e15
    assert 0 < sing.sum() < n and not sing[0]
    r = tm.measureMonteCarlo(ckt, measures, tol=tol, n=n, seed=seed, dist="uniform", quantiles=pt.PROBS, full=True, backend=HipBackend(inst_per_wg=2))
    assert r["n_singular"] == sing.sum() and r["n_stopped"] == 0 and r["n_valid"] == n - sing.sum()
    j = r["names"].index("p.avg")
    want = np.array([1.0 / v["R1"] for v in vals])
    assert np.isnan(r["x"][sing]).all() and (np.abs(r["x"][~sing, j] - want[~sing]) <= 1e-9 * want[~sing] + 1e-12).all()
    s = r["scalars"]["p.avg"]
    assert s["n_valid"] == n - sing.sum() and s["n_nan"] == 0 and s["worst_low"] == int(np.argmin(np.where(sing, np.inf, want)))
    # on a handle: two per workgroup stop some mates; one per workgroup equals the handle of the drawn values
    tr = ckt.analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    plan = M._Plan(ckt, measures, dt, steps)
    names, sc, root = tm.compile_plan(plan, dt)
    flat = plan.flatten(ckt).replicate(n)
    src = abi.source_table(ckt, dt, steps)
    _, t, icdf, log2K = tm._resolve(ckt, tol, "uniform", 3)
    req = abi.tran_mc_req(log2K, True, seed)

    def run_mc(**kw):
        h = Handle(flat, **kw)
        res = h.run_mc(steps, dt, src, req, t, icdf, sc, None, None, pt.PROBS, plan.reqs, plan.treqs, plan.preqs, want_x=True)
        h.close()
        return res
    two = run_mc(inst_per_wg=2)
    assert two["status"] == abi.ERR_SINGULAR and ((two["inst_status"] == abi.ERR_SINGULAR) <= sing).all() and (two["inst_status"] == -1).any()
    assert (two["stat"][:, 0] == np.count_nonzero(two["inst_status"] == 0)).all()
    one = run_mc(inst_per_wg=1)
    assert one["status"] == abi.ERR_SINGULAR and ((one["inst_status"] == abi.ERR_SINGULAR) == sing).all() and (one["inst_status"][~sing] == 0).all()

    def second(drawn):
        h2 = Handle(drawn, inst_per_wg=1)
        d = h2.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs)
        h2.close()
        d["rows"] = (d["meas"], None, d["power"])
        return d
    ref = pt.run_mc_reference(second, flat, steps, dt, src, req, t, icdf, sc, None, None, pt.PROBS, reducer="numpy")
    assert (one["inst_status"] == ref["inst_status"]).all() and pt.bits_equal(one["x"], ref["x"]).all()
    assert (one["sample"] == ref["sample"]).all() and pt.bits_equal(one["stat"], ref["stat"]).all()
