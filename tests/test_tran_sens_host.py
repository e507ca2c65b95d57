"""Sensitivities and corners of transient measurements without a GPU: the design and the reduction of tran_sens_exec.h through the
CPU harness (tests/tran_sens_host) against their numpy definitions bit for bit, every refusal of the judges, and measureSens /
measureWorstCase on the oracle — closed forms of a divider, a scalar that is not monotone inside its tolerance, the host route
bit for bit, the corner dedupe, a singular perturbed instance and the chain rule of a root field."""
import math

import numpy as np
import pytest

from conftest import golden_netlist, load_golden
from oracle.pyoracle import OracleBackend
from spicey_amd import abi, measure as M, synth
from spicey_amd import tran_mc as tm
from spicey_amd import tran_sens as ts
from spicey_amd.measure import delay, edge, efficiency, measureTRANBatch, power, rise_time, stats, when
from spicey_amd.netlist import parseNetlist
from tran_sens_host import pytsens as ps

OAT = abi.TS_ONE_AT_A_TIME


def _shape(nA):
    """(nR, nC, nL) with nR + nC + nL > nA, all three kinds present."""
    return (nA // 2 + 1, nA // 3 + 2, nA - nA // 2 - nA // 3 + 1)


# ---- the design ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nA", ps.NA)
def test_design_equals_numpy_bit_for_bit_in_both_modes(nA):
    shape = _shape(nA)
    R, Cv, Lv, act, step, lvl, tol = ps.design_inputs(nA, shape, seed=nA)
    assert (np.diff(act) > 1).any() or nA == 1  # act has gaps
    got = ps.design(R, Cv, Lv, abi.tran_sens_req(OAT, nA), act=act, step=step)
    ref = ts.design_values(R, Cv, Lv, act=act, step=step)
    for a, r in zip(got, ref):
        assert a.shape == r.shape and ps.bits_equal(a, r).all()
    g = ts.design_gains(1 + 2 * nA, sum(shape), act, step)
    assert (g[0] == 1.0).all() and np.count_nonzero(g != 1.0) == 2 * nA
    for a in range(nA):
        assert g[1 + 2 * a, act[a]] == 1.0 + step[a] and g[2 + 2 * a, act[a]] == 1.0 - step[a]
    got = ps.design(R, Cv, Lv, abi.tran_sens_req(abi.TS_LEVELS, 0), lvl=lvl, tol=tol)
    ref = ts.design_values(R, Cv, Lv, lvl=lvl, tol=tol)
    for a, r, nom in zip(got, ref, (R, Cv, Lv)):
        assert ps.bits_equal(a, r).all() and ps.bits_equal(a[0], nom[0]).all()  # a row of zeros is the nominal circuit


def test_design_refusals_by_their_text_and_nothing_written():
    R, Cv, Lv, act, step, lvl, tol = ps.design_inputs(3, (3, 2, 1), seed=5)
    ok = abi.tran_sens_req(OAT, 3)
    lv = abi.tran_sens_req(abi.TS_LEVELS, 0)

    def req(mode=OAT, nA=3, **kw):
        q = abi.tran_sens_req(mode, nA)
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    res1 = req()
    res1.reserved[1] = 1

    def refused(match, q=ok, **kw):
        args = dict(act=act, step=step) if q is not None and q.mode == OAT else dict(lvl=lvl, tol=tol)
        args.update(kw)
        with pytest.raises(ps.Refused, match=match) as e:
            ps.design(R, Cv, Lv, q, **args)
        assert str(e.value).startswith("tran sens: "), str(e.value)

    refused("null request", q=None, act=act, step=step)
    refused("struct_bytes", q=req(struct_bytes=8))
    refused("reserved", q=res1)
    refused("unknown mode", q=req(mode=2))
    refused("n_inst = 1 \\+ 2 nA", q=req(nA=2))
    refused("nA >= 1", q=req(nA=0))
    refused("n_inst >= 1", n_inst=0)
    refused("16384", n_inst=16385)
    refused("nR, nC, nL", nR=-1)
    refused("strictly ascending", act=[0, 2, 2])
    refused("strictly ascending", act=[3, 2, 4])
    refused("out of range", act=[0, 2, 6])
    refused("out of range", act=[-1, 2, 5])
    for bad in (0.0, 1.0, -1e-3, np.nan, np.inf):
        refused("step", step=[1e-3, bad, 1e-3])
    refused("null buffer", act=None)
    refused("null buffer", step=None)
    refused("null buffer", have_work=False)
    refused("workspace too small", work_bytes=8)
    refused("LEVELS needs nA = 0", q=req(mode=abi.TS_LEVELS, nA=1))
    for bad in (-0.01, 1.0, np.nan, np.inf):
        t = tol.copy()
        t[2] = bad
        refused("tolerance", q=lv, tol=t)
    for bad in (2, -2, 127):
        l2 = lvl.copy()
        l2[6, 5] = bad
        refused("level", q=lv, lvl=l2)
    refused("null buffer", q=lv, lvl=None)
    refused("null buffer", q=lv, tol=None)
    refused("workspace too small", q=lv, work_bytes=8)
    with pytest.raises(ps.Refused, match="no element"):
        ps.design(np.zeros((7, 0)), np.zeros((7, 0)), np.zeros((7, 0)), ok, act=act, step=step)
    W = ps.lib().spicey_ts_host_workspace_bytes
    assert W(0, 1, 3, 1) == -1 and W(16385, 1, 3, 1) == -1 and W(3, 0, 3, 1) == -1 and W(3, 1, 0, 1) == -1 and W(3, 1, 3, -1) == -1 and W(3, 2, 3, 1) > 0


# ---- the reduction ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nA", ps.NA)
def test_reduction_equals_numpy_bit_for_bit_at_every_thread_count(nA):
    for ns in ps.NS:
        for c, case in enumerate(ps.CASES):
            rows, sc, valid, step, tol = ps.case_inputs(case, nA, ns, seed=1000 * nA + 10 * ns + c)
            rx = tm.eval_reference_scalars(sc, rows, valid)
            rsens, rsign, rbound = ts.reduce_reference_tran_sens(rx, valid, step, tol)
            for threads in ps.THREADS:
                x, sens, sign, bound = ps.reduce(rows, sc, valid, step, tol, threads=threads)
                assert ps.bits_equal(x, rx).all(), (ns, case, threads)
                assert ps.bits_equal(sens, rsens).all() and (sign == rsign).all() and ps.bits_equal(bound, rbound).all(), (ns, case, threads)
            # what the cases are about
            if case == "all_nan":
                assert np.isnan(rbound[0, 0]) and rbound[0, 3] == 0 and rbound[0, 4] == -1 and (rsign[0] == 0).all() and rbound[0, 1] == 0.0
                assert (rsens[0].view(np.uint64) == 0x7FF8000000000000).all()
            elif case == "invalid_perturbed":
                a = nA // 2
                assert np.isnan(rsens[:, a]).all() and (rsign[:, a] == 0).all() and (rbound[:, 3] == nA - (2 if nA > 2 and a != 0 else 1)).all()
            elif case == "equal_pair":
                assert (rsens[:, nA - 1, 0] == 0.0).all() and (rsign[:, nA - 1] == 0).all() and (rbound[:, 3] == nA).all()
            elif case == "ties":
                assert rbound[0, 4] == 0 and rsens[0, 0, 0] == rsens[0, nA - 1, 0] == 1024.0 and rbound[0, 5] == 128.0
            elif case == "interior":
                assert rbound[0, 6] == 1 and rsens[0, 0, 0] == 0.125 and rsens[0, 0, 1] == 2.0
                if nA > 1:
                    assert rsens[0, nA - 1, 0] == 0.25 and rsens[0, nA - 1, 1] == 2.0  # |d| = |c| t: strict <, not counted


def test_reduction_refusals_by_their_text_and_nothing_written():
    rows, sc, valid, step, tol = ps.case_inputs("plain", 3, 2, seed=3)

    def refused(match, **kw):
        args = dict(rows=rows, scalars=sc, valid=None, step=step, tol_act=tol)
        args.update(kw)
        with pytest.raises(ps.Refused, match=match) as e:
            ps.reduce(**args)
        assert str(e.value).startswith("tran sens: "), str(e.value)

    refused("n_inst = 1 \\+ 2 nA", nA=2)
    refused("nA >= 1", nA=0)
    refused("bad counts", n_inst=0)
    for bad in (0.0, 1.0, np.nan, -np.inf):
        refused("step", step=[1e-3, 1e-3, bad])
    for bad in (-1e-9, 1.0, np.nan, np.inf):
        refused("tolerance", tol_act=[0.1, bad, 0.1])
    refused("null buffer", step=None, nA=3)
    refused("null buffer", tol_act=None)
    refused("null buffer", have_out=False)
    refused("workspace too small", work_bytes=8)
    # everything the scalar judge refuses, under this call's prefix
    F, K, ADD, GUARD = tm.F, tm.K, tm.ADD, tm.GUARD
    for prog in ([ADD], [K(1.0)] * 5 + [ADD] * 4, [F(0, 0, 0), F(0, 0, 1)], [F(0, 0, 0), GUARD], [(9, 0, 0, 0, 0.0)], [F(3, 0, 0)], [F(0, 2, 0)], [F(0, 0, 8)], [F(1, 0, 0)],
                 [K(np.inf)], [(abi.MCOP_CONST, 0, 0, 1, 1.0)]):
        refused("tran sens: ", scalars=tm.make_scalars([[F(0, 0, 7)], prog], check=False))
    bad = sc.copy()
    bad["reserved"][1] = 1
    refused("reserved", scalars=bad)
    x, sens, sign, bound = ps.reduce(rows, sc, None, step, tol)  # the good one goes through
    assert ps.bits_equal(x[:, 0], rows[0][:, 0, 7]).all() and (bound[:, 3] == 3).all()


# ---- the public interface ---------------------------------------------------------------------------------------------------
DIVIDER = "V1 in 0 5\nR1 in out 1000\nR2 out 0 2000\n.tran 1e-6 1e-5\n.end\n"
RC_PULSE = "V1 in 0 PULSE(0 5 1e-6 1e-7 1e-7 2e-5 4e-5)\nR1 in out 1000\nC1 out 0 2e-9\nR2 out 0 100000\n.tran 4e-7 4e-5\n.end\n"
# a series RLC driven by a step: the output at the end of the run sits near the first peak of the ringing, whose instant moves with L
RLC = "V1 in 0 1\nR1 in a 10\nL1 a out 1e-3\nC1 out 0 1e-6\n.tran 1e-6 1e-4\n.end\n"


def test_divider_sensitivities_and_corners_against_the_closed_form():
    ckt = parseNetlist(DIVIDER)
    V, R1, R2, t, h = 5.0, 1000.0, 2000.0, 0.05, 1e-3
    r = ts.measureWorstCase(ckt, {"o": stats("v(out)")}, tol={"R": t}, rel_step=h, backend=ps.HostTranSensBackend())
    s = r["scalars"]["o.final"]
    dln = V * R1 * R2 / (R1 + R2) ** 2  # dv / d ln R2 = -dv / d ln R1
    # central-difference truncation (h^2 R^2 / (R1 + R2)^2 < h^2 here) plus the parity bar 1e-9 on x over the step 2 h
    rel = h * h + 1e-9 / (2.0 * h)
    assert abs(s["sens"]["R1"] + dln) <= rel * dln and abs(s["sens"]["R2"] - dln) <= rel * dln, s["sens"]
    assert abs(s["nominal"] - V * R2 / (R1 + R2)) <= 1e-9 * V
    assert abs(s["wc"] - 2 * dln * t) <= rel * 2 * dln * t and abs(s["rss"] - math.sqrt(2.0) * dln * t) <= rel * 2 * dln * t
    assert s["linear_low"] == s["nominal"] - s["wc"] and s["linear_high"] == s["nominal"] + s["wc"]
    assert s["ranking"] == ["R1", "R2"] or s["ranking"] == ["R2", "R1"]
    assert s["dominant"] in ("R1", "R2") and s["n_nan"] == 0 and s["n_interior"] == 0 and s["monotone"] is True
    hi = V * R2 * (1 + t) / (R1 * (1 - t) + R2 * (1 + t))
    lo = V * R2 * (1 - t) / (R1 * (1 + t) + R2 * (1 - t))
    assert abs(s["corner_high"] - hi) <= 1e-9 * hi and abs(s["corner_low"] - lo) <= 1e-9 * lo
    k_hi, k_lo = r["corner_index"]["o.final"]
    assert (r["corner_levels"][k_hi] == [-1, 1]).all() and (r["corner_levels"][k_lo] == [1, -1]).all()  # the signs are exactly (-1, +1)
    assert s["corner_high_values"] == {"R1": R1 * (1.0 + -1.0 * t), "R2": R2 * (1.0 + t)} and s["corner_low_values"] == {"R1": R1 * (1.0 + t), "R2": R2 * (1.0 + -1.0 * t)}
    assert s["corner_low"] < s["linear_low"] * (1 + 1e-2) and s["corner_low"] < s["nominal"] < s["corner_high"]
    assert r["elements"] == ["R1", "R2"] and r["active"] == ["R1", "R2"] and r["tol"] == [t, t] and r["n_singular"] == 0
    # min, max, avg, first, final of the DC output share their corners; pp is constant zero: its corners are the nominal row
    assert r["corner_index"]["o.max"] == (k_hi, k_lo) and r["corner_index"]["o.avg"] == (k_hi, k_lo) and r["corner_index"]["o.pp"] == (0, 0)
    assert r["n_corners"] == len(r["corner_levels"]) - 1 <= 4


def test_a_scalar_that_is_not_monotone_inside_the_tolerance_says_so():
    ckt = parseNetlist(RLC)
    r = ts.measureWorstCase(ckt, {"o": stats("v(out)")}, tol={"L1": 0.2}, backend=ps.HostTranSensBackend())
    s = r["scalars"]["o.final"]
    assert s["n_interior"] >= 1 and s["monotone"] is False, s
    # the oracle agrees: at the fitted parabola's vertex, inside the interval, the scalar exceeds both corners
    d, c = s["sens"]["L1"], s["curvature"]["L1"]
    u = -d / c
    assert c < 0 and abs(u) < 0.2
    inner = M.measureTRAN(parseNetlist(RLC.replace("1e-3", repr(1e-3 * (1.0 + u)))), {"o": stats("v(out)")}, backend=OracleBackend())["o"]["final"]
    assert inner > max(s["corner_low"], s["corner_high"]) and inner > s["nominal"]


def test_corner_rows_dedupe_and_map_back():
    sign = np.array([[1, -1, 0], [1, -1, 0], [-1, 1, 0], [0, 0, 0], [1, 1, 1]], np.int8)
    act = np.array([0, 2, 5])
    lvl, idx = ts.corner_rows(sign, act, 6)
    assert lvl.dtype == np.int8 and (lvl[0] == 0).all() and len(lvl) == 5  # nominal, (+-0), (-+0), (+++), (---)
    assert len({row.tobytes() for row in lvl}) == len(lvl)
    for j in range(len(sign)):
        hi, lo = idx[j]
        assert (lvl[hi][act] == sign[j]).all() and (lvl[lo][act] == -sign[j]).all()
        assert (np.delete(lvl[hi], act) == 0).all() and (np.delete(lvl[lo], act) == 0).all()
    assert (idx[0] == idx[1]).all() and (idx[2] == idx[0][::-1]).all() and (idx[3] == 0).all()


def _variants(text, ckt, tol, n, rel_step=ts.DEFAULT_REL_STEP, levels=None):
    out = []
    for s in range(n):
        c = parseNetlist(text)
        vals = ts.design_circuit(ckt, tol, s, rel_step, levels)
        for e in c.R:
            e.R = vals[e.name]
        for e in c.C:
            e.C = vals[e.name]
        for e in c.L:
            e.L = vals[e.name]
        out.append(c)
    return out


def _batch_x(batch, names):
    return np.array([[np.nan if b[nm.split(".")[0]][nm.split(".")[1]] is None else float(b[nm.split(".")[0]][nm.split(".")[1]]) for nm in names] for b in batch])


def _same(a, b):
    return (np.isnan(a) == np.isnan(b)).all() and ps.bits_equal(a[~np.isnan(a)], b[~np.isnan(b)]).all()


def _end_to_end(text, measures, tol):
    ckt = parseNetlist(text)
    r = ts.measureWorstCase(ckt, measures, tol=tol, full=True, backend=ps.HostTranSensBackend())
    names, nA = r["names"], len(r["active"])
    assert r["x"].shape == (1 + 2 * nA, len(names))
    want = _batch_x(measureTRANBatch(_variants(text, ckt, tol, 1 + 2 * nA), measures, backend=OracleBackend()), names)
    assert _same(r["x"], want)
    lv = r["corner_levels"]
    want_c = _batch_x(measureTRANBatch(_variants(text, ckt, tol, len(lv), levels=lv), measures, backend=OracleBackend()), names)
    assert _same(r["corner_x"], want_c)
    # the sensitivities are the numpy reduction of the scalars as they went down (the squares for the root fields)
    tr = ckt.analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    _, _, root = tm.compile_plan(M._Plan(ckt, measures, dt, steps), dt)
    act = [r["elements"].index(nm) for nm in r["active"]]
    down = np.where(root[None, :], want * want, want)
    sens, sign, bound = ts.reduce_reference_tran_sens(down, None, r["rel_step"], np.asarray(r["tol"])[act])
    for j, nm in enumerate(names):
        s = r["scalars"][nm]
        assert s["n_interior"] == int(bound[j, 6]) and s["n_nan"] == nA - int(bound[j, 3]) and s["monotone"] == (bound[j, 6] == 0), nm
        hi, lo = r["corner_index"][nm]
        assert (lv[hi][act] == sign[j]).all() and (lv[lo][act] == -sign[j]).all(), nm
        if not root[j]:
            assert _same(np.array([np.nan if v is None else v for v in s["sens"].values()]), sens[j, :, 0]), nm
            assert _same(np.array([np.nan if v is None else v for v in s["curvature"].values()]), sens[j, :, 1]), nm
            assert s["wc"] == bound[j, 1] and s["rss"] == math.sqrt(bound[j, 2]), nm
            assert s["dominant"] == (r["active"][int(bound[j, 4])] if bound[j, 4] >= 0 else None), nm
    return r


def test_end_to_end_rc_ladder_equals_the_host_route_bit_for_bit():
    text = synth.rc_ladder(5, seed=3, tran=".tran 1e-9 6e-8")  # 4 RC nodes behind the source
    measures = {"s": stats("v(n5)"), "tr": rise_time("v(n3)"), "d": delay(edge("v(n2)", M.rel(0.5)), edge("v(n5)", M.rel(0.5))), "p": power("R1")}
    r = _end_to_end(text, measures, {"R": 0.02, "C": 0.05})
    assert len(r["active"]) == 8 and r["scalars"]["d.delay"]["dominant"] is not None


def test_end_to_end_boost_probe_equals_the_host_route_bit_for_bit():
    text = golden_netlist(load_golden("boost_probe"))
    measures = {"ripple": stats("v(n3)", t_from=0.05), "rise": when("v(n3)", 5.5), "pl": power("RR1"),
                "eff": efficiency(power("RR1"), power("Vsimulation_voltage_source_0"))}
    r = _end_to_end(text, measures, {"L": 0.05, "C": 0.10})
    assert r["scalars"]["ripple.pp"]["wc"] > 0


def test_a_singular_perturbed_instance_makes_that_elements_entries_none():
    """An island grounded through 0.97e15 ohm, stepped by 5 %: the instance with R2 (1 + h) above 1e15 ohm (1 / R below EPS) is
    singular, the one below is not.  The nominal circuit runs, so R1's entries are there and R2's are None."""
    ckt = parseNetlist("V1 a 0 dc 1\nR1 a 0 1k\nR2 x 0 0.97e15\n.tran 1u 5u\n.end\n")
    measures = {"s": stats("v(a)"), "p": power("R1")}
    r = ts.measureWorstCase(ckt, measures, tol={"R1": 0.02, "R2": 0.05}, rel_step={"R2": 0.05}, full=True, backend=ps.HostTranSensBackend())
    assert r["n_singular"] == 1 and r["rel_step"] == [1e-3, 0.05] and np.isnan(r["x"][3]).all() and not np.isnan(r["x"][4]).any()
    for nm in r["names"]:
        s = r["scalars"][nm]
        assert s["sens"]["R2"] is None and s["n_nan"] == 1 and s["sens"]["R1"] is not None and s["dominant"] == "R1" and s["ranking"] == ["R1"], nm
        if s["curvature"] is not None:
            assert s["curvature"]["R2"] is None
    p = r["scalars"]["p.avg"]
    assert abs(p["sens"]["R1"] + 1e-3) <= (1e-6 + 1e-9 / 2e-3) * 1e-3  # p = 1 / R1: dp / d ln R1 = -p, truncation h^2
    # R2's sign is 0, so it stays nominal in every corner, and the corners run
    assert (r["corner_levels"][:, 1] == 0).all() and p["corner_high"] is not None and p["corner_low"] is not None and r["n_corner_singular"] == 0
    # a singular nominal circuit is the call's error
    from spicey_amd.simulate import SingularMatrixError
    with pytest.raises(SingularMatrixError):
        ts.measureSens(parseNetlist("V1 a 0 dc 1\nR1 a 0 1k\nR2 x 0 1e16\n.tran 1u 5u\n.end\n"), {"s": stats("v(a)")}, tol={"R": 0.01}, backend=ps.HostTranSensBackend())


def test_root_fields_take_the_chain_rule():
    """rms goes down as its square; d, wc and rss come back through d / (2 sqrt(x0)).  Against the direct central difference of
    the rms itself: with s = sqrt(x), the two differ by h^2 (s''' - x''' / (2 s)) / 6 = s' h^2 (-c / (4 x0) + d^2 / (8 x0^2)), d and
    c the square's; twice that for the neglected higher orders, plus the parity bar 1e-9 over the step 2 h."""
    ckt = parseNetlist(RC_PULSE)
    h = 1e-3
    r = ts.measureSens(ckt, {"s": stats("v(out)")}, tol={"R": 0.05, "C": 0.1}, rel_step=h, full=True, backend=ps.HostTranSensBackend())
    j = r["names"].index("s.rms")
    s = r["scalars"]["s.rms"]
    assert s["curvature"] is None and s["nominal"] == r["x"][0, j] > 0
    sq = r["x"][:, j] ** 2
    wc = 0.0
    for a, nm in enumerate(r["active"]):
        direct = (r["x"][1 + 2 * a, j] - r["x"][2 + 2 * a, j]) / (2 * h)
        d2, c2 = (sq[1 + 2 * a] - sq[2 + 2 * a]) / (2 * h), (sq[1 + 2 * a] + sq[2 + 2 * a] - 2 * sq[0]) / (h * h)
        rel = 2 * h * h * (abs(c2) / (4 * sq[0]) + d2 * d2 / (8 * sq[0] ** 2)) + 1e-9 / (2 * h) * r["x"][0, j] / max(abs(direct), 1e-300)
        assert abs(s["sens"][nm] - direct) <= rel * abs(direct), (nm, s["sens"][nm], direct)
        wc += abs(s["sens"][nm]) * r["tol"][r["elements"].index(nm)]
    assert abs(s["wc"] - wc) <= 1e-12 * wc and s["linear_high"] == s["nominal"] + s["wc"]
    # where the nominal square is not positive there is no chain rule
    flat = parseNetlist("V1 in 0 0\nR1 in out 1000\nR2 out 0 2000\n.tran 1e-6 1e-5\n.end\n")
    z = ts.measureSens(flat, {"o": stats("v(out)")}, tol={"R": 0.05}, backend=ps.HostTranSensBackend())["scalars"]["o.rms"]
    assert z["nominal"] == 0.0 and z["wc"] is None and z["rss"] is None and all(v is None for v in z["sens"].values())


def test_the_calls_refuse_what_they_do_not_reduce():
    ckt = parseNetlist(DIVIDER)
    be = ps.HostTranSensBackend()
    for fn in (ts.measureSens, ts.measureWorstCase):
        for name, spec in (("f", M.fourier("v(out)", 1e5)), ("sp", M.spectrum("v(out)", n=8)), ("t", M.trace("v(out)")), ("fi", M.find("v(out)", at=1e-6))):
            with pytest.raises(TypeError, match=type(spec).__name__.lower()):
                fn(ckt, {name: spec}, backend=be)
        with pytest.raises(ValueError, match="nothing to vary"):
            fn(ckt, {"o": stats("v(out)")}, tol={"C": 0.1}, backend=be)
        with pytest.raises(ValueError, match="relative step"):
            fn(ckt, {"o": stats("v(out)")}, rel_step=1.0, backend=be)
        with pytest.raises(ValueError, match="rel_step names"):
            fn(ckt, {"o": stats("v(out)")}, rel_step={"Q1": 1e-3}, backend=be)
        with pytest.raises(ValueError, match="tol >= 1"):
            fn(ckt, {"o": stats("v(out)")}, tol={"R": 1.0}, backend=be)
        assert fn(parseNetlist("V1 in 0 5\nR1 in 0 1\n.end\n"), {"o": stats("v(in)")}, backend=be) is None
    import spicey_amd
    assert spicey_amd.measureSens is ts.measureSens and spicey_amd.measureWorstCase is ts.measureWorstCase
