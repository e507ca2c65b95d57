"""Monte Carlo of transient runs on the CPU: the key order, the scalar programs and the reduction of tran_mc_exec.h through the
harness of tests/tran_mc_host against their numpy definitions (spicey_amd/tran_mc.py) bit for bit, the compiled programs against
measure.derive*, every refusal of the two judges, measureMonteCarlo on a resistive divider against its closed form, and end to
end through HostTranMcBackend against measureTRANBatch over mc_values' variants.

Bars: bit identity everywhere except the closed form, which is held to the project's parity bar 1e-9 |ref| + 1e-12."""
import math

import numpy as np
import pytest

from conftest import golden_netlist, load_golden
from oracle.pyoracle import OracleBackend
from spicey_amd import abi, measure as M
from spicey_amd import tran_mc as tm
from spicey_amd.mc import draw_reference_mc, mc_values
from spicey_amd.measure import cross, delay, edge, efficiency, measureTRANBatch, power, rise_time, settle, stats, when
from spicey_amd.netlist import parseNetlist
from tran_mc_host import pytmc as pt


def test_key_order_is_the_stated_total_order():
    sub = 5e-324
    x = np.array([np.nan, 3.5, -0.0, np.inf, 0.0, -sub, sub, -np.inf, -2.0, -np.nan, 1e-310, -1e-310, 2.0, -3.5, np.nan])
    x.view(np.uint64)[-1] = 0x7FF0000000000001  # a signalling NaN with the smallest payload
    k, back = pt.keys(x)
    assert (k == tm.sort_keys(x)).all()
    order = np.argsort(k, kind="stable")
    want = [-np.inf, -3.5, -2.0, -1e-310, -sub, -0.0, 0.0, sub, 1e-310, 2.0, 3.5, np.inf]
    got = x[order]
    assert pt.bits_equal(got[:len(want)], np.array(want)).all() and np.isnan(got[len(want):]).all() and len(got) == len(want) + 3
    assert (k[np.isnan(x)] == tm.NAN_KEY).all() and (k < tm.PAD_KEY).all()
    assert pt.bits_equal(back[~np.isnan(x)], x[~np.isnan(x)]).all() and pt.bits_equal(back[np.isnan(x)], np.full(3, np.nan)).all()
    assert pt.bits_equal(tm.unsort_keys(k), back).all()
    # strictly increasing keys for increasing numbers, random
    r = np.sort(np.random.default_rng(1).normal(0, 1, 1000) * 10.0 ** np.random.default_rng(2).uniform(-300, 300, 1000))
    kr = pt.keys(r)[0]
    assert (np.diff(kr.astype(object)) >= 0).all() and (np.diff(kr.astype(object))[np.diff(r) > 0] > 0).all()


@pytest.mark.parametrize("ni", (1, 65))
def test_scalar_programs_equal_the_numpy_definition_bit_for_bit(ni):
    rows = pt.rows_like(ni, seed=3 + ni)
    sc = pt.programs_like(12)
    valid = None if ni == 1 else pt.case_inputs("third_invalid", ni, 1, 0)[2]
    x, _, _ = pt.reduce(rows, sc, valid)
    ref = tm.eval_reference_scalars(sc, rows, valid)
    assert pt.bits_equal(x, ref).all()
    if ni > 1:
        assert np.isnan(x).any() and np.isfinite(x).any() and np.isinf(x).any()
        assert pt.bits_equal(x[np.isnan(x)], np.full(int(np.isnan(x).sum()), np.nan)).all()  # one NaN, whatever produced it


def test_guard_and_division_by_zero():
    rows = (np.array([[[1.0, 0.0, -0.0, -1.0, np.nan, 2.0, 0.0, 0.0]]]), None, None)
    F, K, DIV, GUARD = tm.F, tm.K, tm.DIV, tm.GUARD
    progs = [[F(0, 0, f), GUARD, K(7.0)] for f in range(5)] + [[F(0, 0, 5), F(0, 0, 1), DIV], [F(0, 0, 3), F(0, 0, 2), DIV], [F(0, 0, 1), F(0, 0, 2), DIV],
                                                                [K(0.0), F(0, 0, 1), DIV, GUARD, K(1.0)], [K(0.0), F(0, 0, 3), DIV, GUARD, K(1.0)]]
    sc = tm.make_scalars(progs)
    x, _, _ = pt.reduce(rows, sc)
    want = np.array([[7.0, 7.0, 7.0, np.nan, np.nan, np.inf, np.inf, np.nan, np.nan, 1.0]])
    assert pt.bits_equal(x, want).all() and pt.bits_equal(tm.eval_reference_scalars(sc, rows), want).all()


def _plan_and_rows(seed, ni=40):
    """A plan with every supported measure and seeded rows that keep what the passes guarantee (counts are whole numbers >= 0,
    crossing indices -1 or >= 0); the two crossing times of a cross row come in either order and equal, whatever the count."""
    ckt = parseNetlist(RC_PULSE)
    tr = ckt.analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    out, el = "v(out)", "R1"
    measures = {"s": stats(out), "s1": stats(out, t_from=dt * 3, t_to=dt * 3), "c": cross(out, 0.5), "w": when(out, 0.5), "d": delay(edge(out, 0.2), edge(out, 0.8)),
                "tr": rise_time(out), "st": settle(out), "p": power(el), "p1": power(el, t_from=dt * 2, t_to=dt * 2), "e": efficiency(power(el), power(ckt.V[0].name))}
    plan = M._Plan(ckt, measures, dt, steps)
    rng = np.random.default_rng(seed)
    meas = rng.normal(0, 1, (ni, len(plan.reqs), 8))
    for k, r in enumerate(plan.reqs):
        if int(r["kind"]) == abi.MEAS_CROSS:
            cnt = rng.integers(0, 5, ni).astype(float)
            tf = rng.uniform(0, 1e-3, ni)
            meas[:, k, 0], meas[:, k, 1], meas[:, k, 2] = cnt, tf, np.where(np.arange(ni) % 3 == 0, tf, tf + rng.uniform(-1e-3, 1e-3, ni))
    tim = rng.normal(0, 1, (ni, len(plan.treqs), 8))
    tim[:, :, 0], tim[:, :, 3] = rng.integers(-1, 3, tim.shape[:2]), rng.integers(-1, 3, tim.shape[:2])
    tim[:, :, 6], tim[:, :, 7] = rng.integers(0, 4, tim.shape[:2]), rng.integers(0, 4, tim.shape[:2])
    pw = rng.normal(0, 1, (ni, len(plan.preqs), abi.POWER_ROW))
    pw[::5, -1, 4:7] = 0.0  # p_source == 0 in some samples
    return plan, dt, (meas, tim, pw)


RC_PULSE = "V1 in 0 PULSE(0 5 1e-6 1e-7 1e-7 2e-5 4e-5)\nR1 in out 1000\nC1 out 0 2e-9\nR2 out 0 100000\n.tran 2e-7 4e-5\n.end\n"


def test_compiled_programs_equal_derive_bit_for_bit():
    plan, dt, rows = _plan_and_rows(11)
    names, sc, root = tm.compile_plan(plan, dt)
    x, _, _ = pt.reduce(rows, sc)
    assert pt.bits_equal(x, tm.eval_reference_scalars(sc, rows)).all()
    got = tm.finish(x, root[None, :])
    seen_none = 0
    for s in range(rows[0].shape[0]):
        vals = plan.values({"meas": rows[0], "timing": rows[1], "power": rows[2]}, s, dt)
        for j, nm in enumerate(names):
            m, f = nm.split(".")
            want = vals[m][f]
            seen_none += want is None
            want = np.nan if want is None else float(want)
            assert pt.bits_equal(np.array([got[s, j]]), np.array([want])).all() or (math.isnan(want) and math.isnan(got[s, j])), (s, nm, got[s, j], want)
    assert seen_none > 0
    # every numeric field of every supported measure is a scalar, except the ones the module text names
    vals = plan.values({"meas": rows[0], "timing": rows[1], "power": rows[2]}, 0, dt)
    missing = {f"{m}.{f}" for m, d in vals.items() for f in d} - set(names)
    assert missing == {"st.t", "p.apparent", "p.pf", "p1.apparent", "p1.pf"}, missing


@pytest.mark.parametrize("ns", pt.REDUCE_NS)
@pytest.mark.parametrize("ni", pt.REDUCE_NI)
def test_reduction_equals_the_numpy_definition_bit_for_bit(ni, ns):
    for c, case in enumerate(pt.CASES):
        rows, sc, valid, lo, hi = pt.case_inputs(case, ni, ns, seed=100 * ni + ns + c)
        ref_x = tm.eval_reference_scalars(sc, rows, valid)
        ref_sample, ref_stat = tm.reduce_reference_tran_mc(ref_x, valid, lo, hi, pt.PROBS)
        for threads in (0,) + pt.THREADS:
            x, stat, sample = pt.reduce(rows, sc, valid, lo, hi, pt.PROBS, threads=threads)
            assert pt.bits_equal(x, ref_x).all() and (sample == ref_sample).all(), (case, threads)
            assert pt.bits_equal(stat, ref_stat).all(), (case, threads, stat, ref_stat)
        if case == "all_nan":
            assert ref_stat[0, 1] == 0 and ref_stat[0, 5] == -1 and np.isnan(ref_stat[0, 8:]).all() and ref_stat[0, 2] == ref_stat[0, 0]
        if case == "all_invalid_but_one":
            assert (ref_stat[:, 0] == 1).all() and (ref_sample[:, 0] == -1).sum() == ni - 1
        if case == "ties" and ni >= 63:
            assert ref_stat[0, 5] == int(np.argmax(ref_x[:, 0] == -2.0)) and ref_stat[0, 6] == int(np.argmax(ref_x[:, 0] == 3.0))
    # no limits at all: only a NaN violates
    rows, sc, valid, _, _ = pt.case_inputs("plain", ni, ns, seed=ni)
    x, stat, sample = pt.reduce(rows, sc, valid, None, None, ())
    assert (stat[:, 2] == np.isnan(x).sum(axis=0)).all() and stat.shape[1] == 8


def test_every_refusal_of_the_reduction_judge():
    rows = pt.rows_like(3, 1)
    F, K, ADD, GUARD = tm.F, tm.K, tm.ADD, tm.GUARD
    good = [F(0, 0, 0)]

    def refused(progs=(good,), match="tran mc: ", **kw):
        sc = tm.make_scalars(list(progs), check=False)
        for mutate in kw.pop("mutate", ()):
            mutate(sc)
        args = dict(rows=rows, scalars=sc, probs=(0.5,))
        args.update(kw)
        with pytest.raises(pt.Refused) as e:
            pt.reduce(args.pop("rows"), args.pop("scalars"), **args)
        assert str(e.value).startswith("tran mc: ") and match in str(e.value), str(e.value)

    refused([[ADD]], "underflow")
    refused([[F(0, 0, 0), GUARD, GUARD]], "underflow")
    refused([[K(1.0)] * 5 + [ADD] * 4], "overflow")
    refused([[F(0, 0, 0), F(0, 0, 1)]], "exactly one value")
    refused([[F(0, 0, 0), GUARD]], "exactly one value")
    refused([[(0, 0, 0, 0, 0.0)]], "unknown opcode")
    refused([[(8, 0, 0, 0, 0.0)]], "unknown opcode")
    refused([[F(1, 0, 0)]], "list is empty", rows=(rows[0], None, rows[2]))
    refused([[F(3, 0, 0)]], "outside measure, timing, power")
    refused([[F(-1, 0, 0)]], "outside measure, timing, power")
    refused([[F(0, 3, 0)]], "row is out of range")
    refused([[F(0, -1, 0)]], "row is out of range")
    refused([[F(0, 0, 8)]], "field is out of range")
    refused([[F(2, 0, 16)]], "field is out of range")
    refused([[K(np.inf)]], "finite")
    refused([[K(np.nan)]], "finite")
    refused([[(abi.MCOP_CONST, 0, 1, 0, 1.0)]], "unused instruction word")
    refused([[(abi.MCOP_FIELD, 0, 0, 0, 1.0)]], "unused instruction word")
    refused([[F(0, 0, 0), F(0, 0, 1), (abi.MCOP_ADD, 1, 0, 0, 0.0)]], "unused instruction word")
    refused(mutate=[lambda sc: sc.__setitem__("reserved", 1)], match="reserved")
    refused(mutate=[lambda sc: sc.__setitem__("n_ins", 0)], match="1 to 48")
    refused(mutate=[lambda sc: sc.__setitem__("n_ins", 49)], match="1 to 48")
    refused(n_inst=0, match="bad counts")
    refused(n_inst=16385, match="16384")
    refused(n_scalar=0, match="bad counts")
    refused(probs=(0.5, 1.5), match="probability")
    refused(probs=(np.nan,), match="probability")
    refused(probs=(-0.1,), match="probability")
    refused(lo=[np.nan], match="NaN")
    refused(hi=[np.nan], match="NaN")
    refused(have_out=False, match="null buffer")
    refused(have_probs=False, match="null buffer")
    refused(have_rows=False, match="null buffer")
    refused(work_bytes=8, match="workspace too small")
    refused(n_rows=(-1, 2, 2), match="a pass needs")
    refused(strides=(0, 8, 16), match="a pass needs")
    refused(rows=(rows[0], None, rows[2]), n_rows=(3, 2, 2), match="a pass needs")
    W = pt.lib().spicey_tmc_host_workspace_bytes
    assert W(0, 1, 3, 0, 1) == -1 and W(16385, 1, 3, 0, 1) == -1 and W(3, 0, 3, 0, 1) == -1 and W(3, 1, 0, 0, 1) == -1 and W(3, 1, 3, 13, 1) == -1 and W(3, 1, 3, 0, -1) == -1
    assert W(3, 2, 3, 10, 4) > 0
    x, stat, sample = pt.reduce(rows, tm.make_scalars([good]), probs=(0.5,))  # the good one goes through
    assert pt.bits_equal(x[:, 0], rows[0][:, 0, 0]).all()


def test_draw_equals_numpy_in_ohms_and_every_refusal_of_the_draw_judge():
    for ni, shape, L in ((1, (1, 0, 0), 0), (2, (3, 2, 1), 1), (65, (64, 1, 65), 10)):
        R, Cv, Lv, tol, icdf = pt.draw_inputs(ni, shape, L, seed=ni)
        for keep in (False, True):
            req = abi.tran_mc_req(L, keep, 0x1234567890ABCDEF)
            got = pt.draw(R, Cv, Lv, tol, icdf, req)
            inv, c, l = draw_reference_mc(R, Cv, Lv, tol, icdf, L, req.seed, keep)
            from spicey_amd.mc import mc_gains
            g = mc_gains(ni, tol, icdf, L, req.seed, keep)
            assert pt.bits_equal(got[0], R * g[:, :shape[0]]).all() and pt.bits_equal(got[1], c).all() and pt.bits_equal(got[2], l).all()
            assert pt.bits_equal(1.0 / got[0], inv).all()  # the quotient the AC draw stores
    R, Cv, Lv, tol, icdf = pt.draw_inputs(3, (4, 2, 1), 3, seed=7)
    ok = abi.tran_mc_req(3, True, 5)

    def req(**kw):
        q = abi.tran_mc_req(3, True, 5)
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    neg, nan, big, dec, inf = tol.copy(), tol.copy(), tol.copy(), icdf.copy(), icdf.copy()
    neg[3], nan[6], big[0], dec[4], inf[8] = -0.01, np.nan, 1.0 / np.abs(icdf).max(), icdf[3] - 1e-9, np.inf
    for q, kw, tl, tab in ((req(struct_bytes=8), {}, tol, icdf), (req(reserved=1), {}, tol, icdf), (req(log2K=13), {}, tol, icdf), (req(log2K=-1), {}, tol, icdf),
                           (None, {}, tol, icdf), (ok, dict(n_inst=0), tol, icdf), (ok, dict(n_inst=16385), tol, icdf), (ok, {}, neg, icdf), (ok, {}, nan, icdf),
                           (ok, {}, big, icdf), (ok, {}, tol, dec), (ok, {}, tol, inf), (ok, {}, None, icdf), (ok, {}, tol, None), (ok, dict(work_bytes=8), tol, icdf),
                           (ok, dict(have_work=False), tol, icdf), (ok, dict(nR=-1), tol, icdf)):
        with pytest.raises(pt.Refused) as e:
            pt.draw(R, Cv, Lv, tl, tab, q, **kw)
        assert str(e.value).startswith("tran mc: "), str(e.value)
    with pytest.raises(pt.Refused, match="no element"):
        pt.draw(np.zeros((3, 0)), np.zeros((3, 0)), np.zeros((3, 0)), tol, icdf, ok)


# ---- the public interface ---------------------------------------------------------------------------------------------------
DIVIDER = "V1 in 0 5\nR1 in out 1000\nR2 out 0 2000\n.tran 1e-6 1e-5\n.end\n"


def test_divider_against_the_closed_form_and_the_exact_yield():
    ckt = parseNetlist(DIVIDER)
    tol, n, seed, probs = {"R": 0.05}, 200, 3, (0.01, 0.5, 0.99)
    ref = np.array([5.0 * v["R2"] / (v["R1"] + v["R2"]) for v in (mc_values(ckt, tol, seed, s) for s in range(n))])
    lim = (3.30, 3.36)
    assert (np.abs(ref - lim[0]) > 1e-6 * lim[0]).all() and (np.abs(ref - lim[1]) > 1e-6 * lim[1]).all()
    bad = ~((ref >= lim[0]) & (ref <= lim[1]))
    assert 0 < bad.sum() < n
    r = tm.measureMonteCarlo(ckt, {"o": stats("v(out)")}, tol=tol, n=n, seed=seed, quantiles=probs, limits={"o.final": lim}, full=True,
                             backend=pt.HostTranMcBackend())
    s = r["scalars"]["o.final"]
    srt = np.sort(ref)
    for p in probs:
        pos = p * (n - 1)
        k = int(pos)
        want = srt[k] + (pos - math.floor(pos)) * (srt[min(k + 1, n - 1)] - srt[k])
        assert abs(s["quantiles"][p] - want) <= 1e-9 * abs(want) + 1e-12, (p, s["quantiles"][p], want)
    assert abs(s["mean"] - ref.mean()) <= 1e-9 * abs(ref.mean()) + 1e-12 and abs(s["std"] - ref.std()) <= 1e-6 * ref.std()
    assert s["n_valid"] == n and s["n_nan"] == 0 and r["n_valid"] == n and r["n_singular"] == 0 and r["n_stopped"] == 0
    assert s["yield"] == 1.0 - bad.sum() / n and r["yield"] == 1.0 - bad.sum() / n
    assert r["failing"] == [(int(k), "o.final") for k in np.nonzero(bad)[0]]
    assert s["worst_low"] == int(np.argmin(ref)) and s["worst_high"] == int(np.argmax(ref))
    assert abs(s["nominal"] - 10.0 / 3.0) <= 1e-9 * 10.0 / 3.0 + 1e-12
    j = r["names"].index("o.final")
    assert (np.abs(r["x"][:, j] - ref) <= 1e-9 * np.abs(ref) + 1e-12).all()


def _host_route(ckt, measures, tol, n, seed, limits, probs):
    """measureTRANBatch over mc_values' variants on the oracle, its values as scalars, reduced by the numpy definition."""
    plan_names = None
    variants = []
    for s in range(n):
        c = parseNetlist(ckt_text(ckt))
        vals = mc_values(c, tol, seed, s)
        for r_ in c.R:
            r_.R = vals[r_.name]
        for c_ in c.C:
            c_.C = vals[c_.name]
        for l_ in c.L:
            l_.L = vals[l_.name]
        variants.append(c)
    out = measureTRANBatch(variants, measures, backend=OracleBackend())
    return out, plan_names


_TEXT = {}


def ckt_text(ckt):
    return _TEXT[id(ckt)]


def _parse(text):
    c = parseNetlist(text)
    _TEXT[id(c)] = text
    return c


def _end_to_end(text, measures, tol, n, seed, limits, expect_nan):
    ckt = _parse(text)
    probs = (0.0, 0.25, 0.5, 1.0)
    r = tm.measureMonteCarlo(ckt, measures, tol=tol, n=n, seed=seed, quantiles=probs, limits=limits, full=True, backend=pt.HostTranMcBackend())
    batch, _ = _host_route(ckt, measures, tol, n, seed, limits, probs)
    tr = ckt.analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    names, sc, root = tm.compile_plan(M._Plan(ckt, measures, dt, steps), dt)
    assert names == r["names"]
    want = np.array([[np.nan if b[nm.split(".")[0]][nm.split(".")[1]] is None else float(b[nm.split(".")[0]][nm.split(".")[1]]) for nm in names] for b in batch])
    assert pt.bits_equal(r["x"], want).all() or (np.isnan(want) == np.isnan(r["x"])).all() and pt.bits_equal(r["x"][~np.isnan(want)], want[~np.isnan(want)]).all()
    lo, hi = tm._limit_arrays(limits, names, root)
    # (the reduction is defined on the scalars as they went down: the squares for the root fields)
    down = np.where(root[None, :], want * want, want)
    ref_sample, ref_stat = tm.reduce_reference_tran_mc(down, None, lo, hi, probs)
    plain = ~root
    for j, nm in enumerate(names):
        s = r["scalars"][nm]
        n_num = int(ref_stat[j, 1])
        assert s["n_valid"] == n and s["n_nan"] == n - n_num and s["yield"] == 1.0 - ref_stat[j, 2] / n, nm
        if plain[j] and n_num:
            assert s["worst_low"] == int(ref_stat[j, 5]) and s["worst_high"] == int(ref_stat[j, 6]), nm
            for q, p in enumerate(probs):
                v = tm._interp(ref_stat[j, 8 + 2 * q], ref_stat[j, 9 + 2 * q], p, n_num, False)
                assert pt.bits_equal(np.array([s["quantiles"][p]]), np.array([v])).all(), (nm, p)
            assert pt.bits_equal(np.array([s["mean"]]), np.array([ref_stat[j, 3] / n_num])).all(), nm
    if limits:
        assert r["failing"] == [(int(k), names[int(ref_sample[k, 1])]) for k in np.nonzero(ref_sample[:, 0] > 0)[0]]
    n_nan = sum(r["scalars"][nm]["n_nan"] for nm in names)
    assert (n_nan > 0) == expect_nan, n_nan
    return r


def test_end_to_end_rc_pulse_equals_the_host_route_bit_for_bit():
    measures = {"tr": rise_time("v(out)", t_to=2e-5), "d": delay(edge("v(in)", 2.5), edge("v(out)", 2.5)), "s": stats("v(out)"), "p": power("R1"),
                "e": efficiency(power("R2"), power("V1"))}
    r = _end_to_end(RC_PULSE, measures, {"R": 0.05, "C": 0.1}, 12, 4, {"s.pp": (None, 4.952), "tr.time": (0, 4.75e-6)}, expect_nan=False)
    assert 0 < len(r["failing"]) < 12


def test_end_to_end_samples_without_a_crossing_count_as_violations():
    """The level sits at the nominal circuit's peak region: some drawn samples never reach it."""
    ckt = _parse(RC_PULSE)
    nominal = M.measureTRAN(ckt, {"s": stats("v(out)")}, backend=OracleBackend())["s"]["max"]
    measures = {"w": when("v(out)", nominal * 0.9995), "s": stats("v(out)")}
    r = _end_to_end(RC_PULSE, measures, {"R": 0.05}, 16, 9, None, expect_nan=True)
    s = r["scalars"]["w.t"]
    assert 0 < s["n_nan"] < 16 and s["yield"] == 1.0 - s["n_nan"] / 16 and r["yield"] == s["yield"]
    assert all(nm == "w.t" for _, nm in r["failing"]) and len(r["failing"]) == s["n_nan"]


def test_end_to_end_boost_probe_equals_the_host_route_bit_for_bit():
    text = golden_netlist(load_golden("boost_probe"))
    measures = {"ripple": stats("v(n3)", t_from=0.05), "rise": when("v(n3)", 5.5), "pl": power("RR1"),
                "eff": efficiency(power("RR1"), power("Vsimulation_voltage_source_0"))}
    r = _end_to_end(text, measures, {"L": 0.05, "C": 0.10}, 16, 1, {"ripple.pp": (None, 1e9), "eff.eff": (0.0, 1.5)}, expect_nan=False)
    assert r["scalars"]["ripple.pp"]["quantiles"][0.0] < r["scalars"]["ripple.pp"]["quantiles"][1.0]


def test_measure_monte_carlo_refuses_what_it_does_not_reduce():
    ckt = parseNetlist(DIVIDER)
    be = pt.HostTranMcBackend()
    for name, spec in (("f", M.fourier("v(out)", 1e5)), ("sp", M.spectrum("v(out)", n=8)), ("t", M.trace("v(out)")), ("sa", M.sample("v(out)", [1e-6])), ("fi", M.find("v(out)", at=1e-6))):
        with pytest.raises(TypeError, match=type(spec).__name__.lower()):
            tm.measureMonteCarlo(ckt, {name: spec}, n=4, backend=be)
    with pytest.raises(ValueError, match="n must be"):
        tm.measureMonteCarlo(ckt, {"o": stats("v(out)")}, n=16385, backend=be)
    with pytest.raises(ValueError, match="no scalar"):
        tm.measureMonteCarlo(ckt, {"o": stats("v(out)")}, n=4, limits={"o.nope": (0, 1)}, backend=be)
    with pytest.raises(ValueError, match="quantile"):
        tm.measureMonteCarlo(ckt, {"o": stats("v(out)")}, n=4, quantiles=(1.5,), backend=be)
    assert tm.measureMonteCarlo(parseNetlist("V1 in 0 5\nR1 in 0 1\n.end\n"), {"o": stats("v(in)")}, n=4, backend=be) is None


def test_no_valid_sample_is_an_error_not_a_division_by_zero():
    """An island grounded through 1e16 ohm is singular in every sample: with keep_first the nominal circuit's error, without it
    the same error for want of any statistic."""
    from spicey_amd.simulate import SingularMatrixError
    ckt = parseNetlist("V1 a 0 dc 1\nR1 a 0 1k\nR2 x 0 1e16\n.tran 1u 5u\n.end\n")
    for keep in (True, False):
        with pytest.raises(SingularMatrixError):
            tm.measureMonteCarlo(ckt, {"s": stats("v(a)")}, tol={"R": 0.01}, n=3, keep_first=keep, backend=pt.HostTranMcBackend())
