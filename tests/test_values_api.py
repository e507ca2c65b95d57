"""trace(), sample(), find() and deriv() through measureTRAN / measureTRANBatch on the CPU: the oracle is a backend without
run_reduced, so the waveforms come from backend.run and the values from reduce_reference_values.  The records' layout, the
trace of an RC pulse and of a DC divider against simulateTRAN's own waveforms bit for bit, sample() against np.interp, find()
on the boost converter against the same thing done by hand, the rules for times, and a dict without these specs on the path
it always took."""
import ctypes as C
import math

import numpy as np
import pytest

from batch_variants import PerInstanceOracle
from conftest import bits_equal, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.measure import (Find, Sample, Trace, _Plan, backend_reduce, cross, deriv, edge, find, fourier, make_value_points, make_value_reqs, measureTRAN,
                                measureTRANBatch, power, rel, sample, stats, time_to_point, trace, when)
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import simulateTRAN

U = 2.0 ** -52
RC = "* pulse into RC\nV1 in 0 PULSE(0 1 0 1u 1u 20u 40u)\nR1 in out 1k\nC1 out 0 1n\n.tran 1u 100u\n.end\n"
DIVIDER = "* DC divider\nV1 in 0 DC 1\nR1 in out 1k\nR2 out 0 3k\n.tran 1u 10u\n.end\n"


def boost_text():
    return golden_netlist(load_golden("boost_probe")).replace(".PRINT TRAN V(n1) V(n3)", ".PRINT TRAN V(n1) V(n2) V(n3)")


def test_the_records_sizes_and_layout():
    assert C.sizeof(abi.SpiceyValReq) == 72 and abi.VAL_REQ_DTYPE.itemsize == 72 and C.sizeof(abi.SpiceyValPoint) == 16 and abi.VAL_POINT_DTYPE.itemsize == 16
    for struct, dtype in ((abi.SpiceyValReq, abi.VAL_REQ_DTYPE), (abi.SpiceyValPoint, abi.VAL_POINT_DTYPE)):
        assert [n for n, _ in struct._fields_] == list(dtype.names)
        assert [dtype.fields[n][1] for n in dtype.names] == [getattr(struct, n).offset for n in dtype.names]
    assert (abi.VAL_TRACE, abi.VAL_POINTS, abi.VAL_FIND, abi.TRACE_MAX_BUCKETS, abi.VAL_TRACE_DOUBLES, abi.VAL_POINT_DOUBLES) == (0, 1, 2, 4096, 6, 4)
    q = make_value_reqs([(2, 1, 3, -1, 0, 4, 5, 6, 7, 8, 9, 10, 11)])[0]
    assert tuple(q) == (2, 1, 3, -1, 0, 4, 5, 6, 7, 8, 9, 10, 11, 0)
    assert tuple(make_value_points([(3, 0.25)])[0]) == (3, 0.25)
    reqs = make_value_reqs([(0, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, 7), (1, 0, 0, -1, 0, 0, -1, 0, 0, 0, 0, 11, 0), (2, 0, 0, -1, 0, 0, -1, 0, 0, 0, 0, 0, 0)])
    assert abi.val_row_doubles(reqs) == 44 and abi.val_row_doubles(reqs[:1]) == 42 and abi.val_row_doubles(reqs[2:]) == 4 and abi.val_row_doubles(reqs[:0]) == 1
    # the struct of spicey_run_reduced: struct_bytes first, the five groups, then the values group
    L = abi.SpiceyReducedLists
    assert C.sizeof(L) == 160 and L._fields_[0][0] == "struct_bytes" and L.struct_bytes.offset == 0
    assert [getattr(L, n).offset for n in ("reqs", "meas", "freqs", "four", "treqs", "timing", "sreqs", "spec", "preqs", "power")] == list(range(8, 88, 8))
    assert [getattr(L, n).offset for n in ("n_req", "n_four", "four_stride", "n_timing", "n_spec", "spec_stride", "n_power", "n_values")] == list(range(88, 120, 4))
    assert [getattr(L, n).offset for n in ("vreqs", "values", "pts", "n_pts", "values_stride", "reserved")] == [120, 128, 136, 144, 152, 156]


def test_spec_arguments():
    assert trace("v(a)") == Trace("v(a)", 512, None, None) and sample("v(a)", [1e-6, 2]) == Sample("v(a)", (1e-6, 2.0))
    e = edge("v(b)", 1.0, "fall")
    assert find("v(a)", when=e, t_from=1e-6) == Find("v(a)", e, None, 1e-6, None, False) and deriv("v(a)", at=2e-6) == Find("v(a)", None, 2e-6, None, None, True)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            trace("v(a)", buckets=bad)
    for bad in ([], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            sample("v(a)", bad)
    for kw in ({}, {"when": e, "at": 1.0}, {"at": float("nan")}, {"at": 1.0, "t_from": 0.0}):
        with pytest.raises(ValueError):
            find("v(a)", **kw)
    with pytest.raises(TypeError):
        find("v(a)", when=when("v(b)", 1.0))


def test_trace_of_the_rc_pulse_is_simulateTRAN_s_waveform(oracle_backend):
    tr = simulateTRAN(parseNetlist(RC), backend=oracle_backend, as_lists=False)
    y, x = tr["nodeVoltages"]["out"], tr["nodeVoltages"]["in"] - tr["nodeVoltages"]["out"]
    cur = tr["elementCurrents"]["C1"]
    n, dt = len(y), 1e-6
    assert n == 101
    m = {"all": trace("v(out)", buckets=1000), "b7": trace("v(out)", buckets=7), "win": trace("v(in,out)", buckets=4, t_from=10e-6, t_to=42.4e-6),
         "i": trace("i(C1)", buckets=101), "one": trace("v(out)", buckets=1), "s": stats("v(out)")}
    got = measureTRAN(parseNetlist(RC), m, backend=oracle_backend)
    assert list(got) == list(m)
    # buckets above the window's sample count: lowered to it, and the waveform itself comes back, in every field and as the polyline
    a = got["all"]
    assert a["buckets"] == n and len(a["t"]) == n
    times = [k * dt for k in range(n)]
    for key in ("first", "min", "max", "last", "v"):
        assert bits_equal(a[key], y).all(), key
    for key in ("t_first", "t_min", "t_max", "t_last", "t"):
        assert a[key] == times, key
    assert bits_equal(got["i"]["v"], cur).all() and got["i"]["t"] == times
    for name, sig, s0, s1, B in (("b7", y, 0, 100, 7), ("win", x, 10, 42, 4), ("one", y, 0, 100, 1)):
        g = got[name]
        nn = s1 - s0 + 1
        assert g["buckets"] == B
        poly = []
        for b in range(B):
            lo, hi = s0 + b * nn // B, s0 + (b + 1) * nn // B - 1
            w = sig[lo:hi + 1]
            kmn, kmx = lo + int(np.argmin(w)), lo + int(np.argmax(w))
            assert (g["t_first"][b], g["t_min"][b], g["t_max"][b], g["t_last"][b]) == (lo * dt, kmn * dt, kmx * dt, hi * dt), (name, b)
            assert bits_equal([g["first"][b], g["min"][b], g["max"][b], g["last"][b]], [sig[lo], sig[kmn], sig[kmx], sig[hi]]).all(), (name, b)
            poly += sorted({lo, kmn, kmx, hi})
        assert g["t"] == [k * dt for k in poly] and bits_equal(g["v"], sig[poly]).all() and len(poly) <= 4 * B
    assert (got["one"]["min"][0], got["one"]["max"][0], got["one"]["t_min"][0], got["one"]["t_max"][0]) == \
        (got["s"]["min"], got["s"]["max"], got["s"]["t_min"], got["s"]["t_max"])
    with pytest.raises(ValueError):
        measureTRAN(parseNetlist(RC), {"t": trace("v(out)", t_from=50e-6, t_to=20e-6)}, backend=oracle_backend)
    with pytest.raises(ValueError):
        measureTRAN(parseNetlist(RC), {"t": trace("v(nope)")}, backend=oracle_backend)
    p = _Plan(parseNetlist(RC), {"t": trace("v(out)", buckets=abi.TRACE_MAX_BUCKETS + 5)}, 1e-6, 100)
    assert int(p.vreqs[0]["buckets"]) == 101
    with pytest.raises(ValueError):
        _Plan(parseNetlist(RC), {"t": trace("v(out)", buckets=abi.TRACE_MAX_BUCKETS + 5)}, 1e-6, 2 * abi.TRACE_MAX_BUCKETS)
    assert int(_Plan(parseNetlist(RC), {"t": trace("v(out)", buckets=abi.TRACE_MAX_BUCKETS)}, 1e-6, 2 * abi.TRACE_MAX_BUCKETS).vreqs[0]["buckets"]) == 4096


def test_sample_against_np_interp_and_the_divider(oracle_backend):
    tr = simulateTRAN(parseNetlist(RC), backend=oracle_backend, as_lists=False)
    y = tr["nodeVoltages"]["out"]
    dt, steps = 1e-6, 100
    grid = np.arange(steps + 1) * dt
    rng = np.random.default_rng(3)
    ts = np.concatenate([[0.0, 100e-6, 7e-6, 7.5e-6, 99.999e-6], rng.uniform(0.0, 100e-6, 40)])
    got = measureTRAN(parseNetlist(RC), {"s": sample("v(out)", ts), "i": sample("i(R1)", ts[:3])}, backend=oracle_backend)["s"]
    # (100e-6 / dt rounds to just above 100: clamped, and reported as the run's last step)
    assert got["t"] == [ts[0], 100 * dt] + ts[2:].tolist() and len(got["value"]) == len(ts)
    for t, v, sl in zip(ts, got["value"], got["slope"]):
        k = min(int(math.floor(t / dt)), steps - 1)
        # a few ulp of the bracketing samples — the product and the sum of either evaluation round once each: 4 U max|y| —
        # plus what the place inside the interval is worth: q = t / dt is off by half an ulp of q, np.interp's t - k dt by an
        # ulp of t and one of the grid point, together less than 3 U q of a step, and a step is worth |y[k+1] - y[k]|
        assert abs(v - float(np.interp(t, grid, y))) <= 4 * U * max(abs(y[k]), abs(y[k + 1])) + 3 * U * (t / dt) * abs(y[k + 1] - y[k]), t
        assert sl == (y[k + 1] - y[k]) / dt
    assert got["value"][0] == y[0] and got["value"][1] == y[100] and got["value"][2] == y[7]  # (on a sample: the sample itself)
    d = measureTRAN(parseNetlist(DIVIDER), {"s": sample("v(out)", [0.0, 3.3e-6, 10e-6]), "t": trace("v(out)", buckets=3), "at": find("v(out)", at=3.3e-6),
                                            "d": deriv("v(out)", at=3.3e-6)}, backend=oracle_backend)
    ref = simulateTRAN(parseNetlist(DIVIDER), backend=oracle_backend, as_lists=False)["nodeVoltages"]["out"]
    assert all(abs(v - 0.75) <= 1e-9 for v in d["s"]["value"]) and d["s"]["slope"] == [(ref[1] - ref[0]) / 1e-6, (ref[4] - ref[3]) / 1e-6, (ref[10] - ref[9]) / 1e-6]
    assert d["t"]["buckets"] == 3 and bits_equal(d["t"]["first"], ref[[0, 3, 7]]).all() and bits_equal(d["t"]["last"], ref[[2, 6, 10]]).all()
    assert d["at"] == {"t": 3.3e-6, "value": d["s"]["value"][1], "slope": d["s"]["slope"][1], "level": None, "count": None}
    assert d["d"] == {"t": 3.3e-6, "value": d["s"]["slope"][1], "slope": d["s"]["slope"][1], "level": None, "count": None}


def test_times_are_clamped_within_half_a_step_and_refused_beyond():
    dt, steps = 1e-6, 100
    assert time_to_point(0.0, dt, steps) == (0, 0.0, 0.0) and time_to_point(100e-6, dt, steps) == (99, 1.0, 100 * dt)
    assert time_to_point(-0.49e-6, dt, steps) == (0, 0.0, 0.0) and time_to_point(100.49e-6, dt, steps) == (99, 1.0, 100 * dt)
    k, f, t = time_to_point(41.25e-6, dt, steps)
    assert (k, t) == (41, 41.25e-6) and f == 41.25e-6 / dt - 41 and 0.0 <= f < 1.0
    assert time_to_point(41e-6, dt, steps)[:2] == (int(math.floor(41e-6 / dt)), 41e-6 / dt - math.floor(41e-6 / dt))
    for bad in (-0.5e-6, -1e-6, 100.5e-6, 1.0, float("nan")):
        with pytest.raises(ValueError):
            time_to_point(bad, dt, steps)
    with pytest.raises(ValueError):
        time_to_point(0.0, dt, 0)
    got = measureTRAN(parseNetlist(RC), {"s": sample("v(out)", [-0.4e-6, 100.4e-6])}, backend=_Oracle())["s"]
    assert got["t"] == [0.0, 100 * dt]
    with pytest.raises(ValueError):
        measureTRAN(parseNetlist(RC), {"s": sample("v(out)", [50e-6, 100.6e-6])}, backend=_Oracle())
    with pytest.raises(ValueError):
        measureTRAN(parseNetlist(RC), {"f": find("v(out)", at=-0.6e-6)}, backend=_Oracle())


def test_find_on_the_boost_converter_equals_the_same_thing_by_hand(oracle_backend):
    text = boost_text()
    tr = simulateTRAN(parseNetlist(text), backend=oracle_backend, as_lists=False)
    sw, out, il = tr["nodeVoltages"]["N2"], tr["nodeVoltages"]["N3"], tr["elementCurrents"]["LL1"]
    dt = 1e-3
    lo, hi = float(sw[20:].min()), float(sw[20:].max())
    level = lo + 0.5 * (hi - lo)
    m = {"valley": find("i(LL1)", when=edge("v(n2)", rel(0.5, t_from=20e-3), "rise"), t_from=20e-3),
         "out": find("v(n3)", when=edge("v(n2)", level, "either", n=-1)),
         "dout": deriv("v(n3)", when=edge("v(n2)", level, "either", n=-1)),
         "never": find("i(LL1)", when=edge("v(n2)", float(sw.max()) + 1.0, "rise")),
         "w": when("v(n2)", level, "either", n=-1), "s": stats("v(n2)")}
    got = measureTRAN(parseNetlist(text), m, backend=oracle_backend)
    assert list(got) == list(m)

    def by_hand(y, k0, dirs, n):
        ks = [k for k in range(k0, 100) if ("fall" in dirs and sw[k] > level >= sw[k + 1]) or ("rise" in dirs and sw[k] < level <= sw[k + 1])]
        k = ks[n - 1] if n > 0 else ks[n]
        f = (level - sw[k]) / (sw[k + 1] - sw[k])
        d = y[k + 1] - y[k]
        return {"t": (k + f) * dt, "value": y[k] if f == 0 else y[k + 1] if f == 1 else y[k] + f * d, "slope": d / dt, "level": level, "count": len(ks)}

    assert got["valley"] == by_hand(il, 20, ("rise",), 1)
    assert got["out"] == by_hand(out, 0, ("fall", "rise"), -1)
    assert got["dout"] == {**got["out"], "value": got["out"]["slope"]}
    assert got["out"]["t"] == got["w"]["t"] and got["out"]["count"] == got["w"]["count"]  # find's t is when()'s, bit for bit
    assert got["never"] == {"t": None, "value": None, "slope": None, "level": float(sw.max()) + 1.0, "count": 0}
    assert got["w"] == measureTRAN(parseNetlist(text), {"w": m["w"]}, backend=oracle_backend)["w"]
    with pytest.raises(ValueError):
        measureTRAN(parseNetlist(text), {"f": find("i(LL1)", when=edge("v(n2)", level), t_from=50e-3, t_to=50e-3)}, backend=oracle_backend)
    # the plan: one hidden targ-only request behind the dict's own timing requests, both signals recorded, currents needed
    ckt = parseNetlist(text)
    p = _Plan(ckt, {"w": m["w"], "valley": m["valley"], "s": sample("v(n3)", [1e-3])}, dt, 100)
    cols = {n: c for c, n in enumerate(p.out_nodes)}
    assert p.need_i and p.out_nodes == sorted([ckt.nodes.get("n2"), ckt.nodes.get("n3")]) and len(p.treqs) == 2 and len(p.vreqs) == 2
    q = p.vreqs[0]
    assert (int(q["kind"]), int(q["signal"]), int(q["x_signal"]), int(q["x_col"]), int(q["x_col_ref"]), int(q["timing_row"])) == (2, 1, 0, cols[ckt.nodes.get("n2")], -1, 1)
    assert int(p.treqs[1]["has_trig"]) == 0 and tuple(p.treqs[1]["targ"])[:6] == (0, cols[ckt.nodes.get("n2")], -1, 1, 1, abi.TIMING_MINMAX)
    assert (int(p.treqs[1]["step_from"]), int(p.treqs[1]["step_to"]), int(p.treqs[1]["targ"]["base_from"])) == (20, 100, 20)
    assert tuple(p.pts[0]) == (1, 0.0) and [(n, k) for n, _, k in p.names] == [("w", 0), ("valley", 0), ("s", 1)]


class _Oracle(PerInstanceOracle):
    """The per-instance oracle (it always computes the currents, and hands them out only when asked)."""

    def run(self, flat, steps, dt, src, want_currents=True, want_iters=True):
        res = super().run(flat, steps, dt, src, True, want_iters)
        if not want_currents:
            res["out_i"] = None
        return res


def _state(ckt):
    return ([c.vPrev for c in ckt.C], [l.iPrev for l in ckt.L], [d.vdPrev for d in ckt.D], [s.isOn for s in ckt.S])


def test_batch_slots_equal_solo_calls():
    from batch_variants import variant
    base = boost_text()
    texts = [variant(base, k) for k in range(3)]
    m = {"t": trace("v(n3)", buckets=16), "f": find("i(LL1)", when=edge("v(n3)", rel(0.5), "rise")), "s": sample("v(n3)", [1.5e-3, 0.05]), "st": stats("v(n3)"),
         "p": power("RR1")}
    batch, solo = [parseNetlist(t) for t in texts], [parseNetlist(t) for t in texts]
    be = _Oracle()
    got = measureTRANBatch(batch, m, backend=be)
    assert [n for n, _ in be.launches] == [3]
    for g, c, b in zip(got, solo, batch):
        assert g == measureTRAN(c, m, backend=_Oracle()) and _state(b) == _state(c)
        assert g["f"]["t"] is not None and g["t"]["buckets"] == 16
    assert len({g["f"]["level"] for g in got}) == 3  # (a level of each circuit's own)


def test_a_dict_without_these_specs_takes_the_path_it_took():
    """The backend sees the call it saw before — never run_reduced —, the result is the object it was, and the batch's grouping
    key is the one it was."""
    calls = []

    class Recorder(_Oracle):
        def _note(self, name, flat, steps, dt, src, lists):
            calls.append((name, [len(lst) for lst in lists]))
            return backend_reduce(_Oracle(), flat, steps, dt, src, *[lists[k] if k < len(lists) else [] for k in range(3)], True,
                                  *[lists[k] if k < len(lists) else [] for k in range(3, 5)])

        def run_measure(self, flat, steps, dt, src, reqs, want_iters=True):
            return self._note("run_measure", flat, steps, dt, src, (reqs,))

        def run_measure_fourier(self, flat, steps, dt, src, reqs, freqs, want_iters=True):
            return self._note("run_measure_fourier", flat, steps, dt, src, (reqs, freqs))

        def run_measure_timing(self, flat, steps, dt, src, reqs, freqs, treqs, want_iters=True):
            return self._note("run_measure_timing", flat, steps, dt, src, (reqs, freqs, treqs))

        def run_measure_power(self, flat, steps, dt, src, reqs, freqs, treqs, sreqs, preqs, want_iters=True):
            return self._note("run_measure_power", flat, steps, dt, src, (reqs, freqs, treqs, sreqs, preqs))

        def run_reduced(self, *a, **k):
            raise AssertionError("a dict without trace() / sample() / find() reached run_reduced")

    s, f, w, pw = {"s": stats("v(out)"), "x": cross("v(out)", 0.5)}, {"f": fourier("v(out)", 1.0 / 40e-6, periods=2)}, {"w": when("v(out)", 0.5)}, {"p": power("R1")}
    for m, want in ((s, ("run_measure", [2])), ({**s, **f}, ("run_measure_fourier", [2, 1])), ({**f, **w}, ("run_measure_timing", [0, 1, 1])),
                    ({**s, **pw}, ("run_measure_power", [2, 0, 0, 0, 1]))):
        calls.clear()
        got = measureTRAN(parseNetlist(RC), m, backend=Recorder())
        assert calls == [want] and got == measureTRAN(parseNetlist(RC), m, backend=_Oracle()) and list(got) == list(m)
    ckt = parseNetlist(RC)
    p = _Plan(ckt, {**s, **f, **w}, 1e-6, 100)
    assert len(p.vreqs) == 0 and len(p.pts) == 0 and p.key() == p.reqs.tobytes() + b"|" + p.freqs.tobytes() + b"|" + p.treqs.tobytes()
    p = _Plan(ckt, {**s, **f, "p": power("C1")}, 1e-6, 100)
    assert p.key() == p.reqs.tobytes() + b"|" + p.freqs.tobytes() + b"|p|" + p.preqs.tobytes()
    q = _Plan(ckt, {**s, **f, "p": power("C1"), "t": trace("v(out)"), "a": find("v(out)", at=3e-6)}, 1e-6, 100)
    assert q.key() == p.key() + b"|v|" + q.vreqs.tobytes() + b"|" + q.pts.tobytes()
    assert _Plan(ckt, {"t": trace("v(out)", buckets=8)}, 1e-6, 100).key() != _Plan(ckt, {"t": trace("v(out)", buckets=9)}, 1e-6, 100).key()
    assert _Plan(ckt, {"a": find("v(out)", at=3e-6)}, 1e-6, 100).key() != _Plan(ckt, {"a": find("v(out)", at=3.5e-6)}, 1e-6, 100).key()
    # with the specs, a backend that has run_reduced gets it, with every list and the point table
    seen = []

    class WithReduced(Recorder):
        def run_reduced(self, flat, steps, dt, src, reqs=(), freqs=(), treqs=(), sreqs=(), preqs=(), vreqs=(), pts=(), want_iters=True):
            seen.append([len(x) for x in (reqs, freqs, treqs, sreqs, preqs, vreqs, pts)])
            return backend_reduce(_Oracle(), flat, steps, dt, src, reqs, freqs, treqs, True, sreqs, preqs, vreqs, pts)

    m = {**s, **w, "t": trace("v(out)", buckets=5), "f": find("i(R1)", when=edge("v(out)", 0.5)), "sm": sample("v(out)", [1e-6, 2e-6, 3.5e-6])}
    calls.clear()
    got = measureTRAN(parseNetlist(RC), m, backend=WithReduced())
    assert seen == [[2, 0, 2, 0, 0, 3, 3]] and calls == [] and got == measureTRAN(parseNetlist(RC), m, backend=_Oracle())
    assert got["f"]["t"] == got["w"]["t"] and got["f"]["level"] == 0.5
