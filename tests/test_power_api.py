"""power() and efficiency() through measureTRAN / measureTRANBatch on the CPU: the oracle is a backend without
run_measure_power, so the waveforms come from backend.run and the products from reduce_reference_power.  The element form's
terminals and sign, a DC divider's powers and efficiency to the parity bar, the energy of a resistor against the trapezoid
of simulateTRAN's own waveforms, the one-sample rules, and a dict without these specs on the path it always took."""
import ctypes as C
import math

import numpy as np
import pytest

from batch_variants import PerInstanceOracle
from conftest import golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.measure import (Efficiency, Power, _Plan, _power_factors, cross, derive_efficiency, derive_power, efficiency, fourier, make_power_reqs,
                                measureTRAN, measureTRANBatch, power, stats, when)
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import simulateTRAN

trapz = getattr(np, "trapezoid", None) or np.trapz
U = 2.0 ** -52
BAR = 1e-9  # the project's parity bar, relative

RC = "* pulse into RC\nV1 in 0 PULSE(0 1 0 1u 1u 20u 40u)\nR1 in out 1k\nC1 out 0 1n\n.tran 1u 100u\n.end\n"
DIVIDER = "* DC divider\nV1 in 0 DC 1\nR1 in out 1k\nR2 out 0 3k\n.tran 1u 10u\n.end\n"
ELEMENTS = ("* one element of every recorded kind\n.MODEL D D\n.MODEL SWMOD SW\nV1 n1 0 DC 5\nL1 n1 n2 1m\nD1 n2 n3 D\nC1 n3 0 10u\nR1 n3 0 1k\n"
            "S1 n2 0 n4 0 SWMOD\nV2 n4 0 PULSE(0 10 0 1n 1n 5u 10u)\nR2 0 n3 2k\nR3 0 0 1k\nr1b n1 n3 5k\nR1B n2 n3 5k\n.tran 1u 20u\n.end\n")


def test_the_request_record_is_48_bytes():
    assert C.sizeof(abi.SpiceyPowerReq) == 48 and abi.POWER_REQ_DTYPE.itemsize == 48 and abi.POWER_REQ is abi.POWER_REQ_DTYPE and abi.POWER_ROW == 16
    assert [n for n, _ in abi.SpiceyPowerReq._fields_] == list(abi.POWER_REQ_DTYPE.names)
    assert [abi.POWER_REQ_DTYPE.fields[n][1] for n in abi.POWER_REQ_DTYPE.names] == [getattr(abi.SpiceyPowerReq, n).offset for n in abi.POWER_REQ_DTYPE.names]
    q = make_power_reqs([(0, 1, 2, 1, 3, -1, 1, 4, 9)])[0]
    assert tuple(q) == (0, 1, 2, 1, 3, -1, 1, 0, 4, 9)


def test_element_form_resolution():
    ckt = parseNetlist(ELEMENTS)
    node = ckt.nodes.get
    # recording order R, C, L, V, S, D: R1 R2 R3 r1b R1B | C1 | L1 | V1 V2 | S1 | D1
    for name, want in (("R1", ((0, node("n3"), 0), (1, 0, 0), 0)), ("c1", ((0, node("n3"), 0), (1, 5, 0), 0)),
                       ("L1", ((0, node("n1"), node("n2")), (1, 6, 0), 0)), ("V1", ((0, node("n1"), 0), (1, 7, 0), 0)),
                       ("v2", ((0, node("n4"), 0), (1, 8, 0), 0)), ("S1", ((0, node("n2"), 0), (1, 9, 0), 0)),
                       ("D1", ((0, node("n2"), node("n3")), (1, 10, 0), 0)),  # nPlus / nMinus
                       (" R2 ", ((0, node("n3"), 0), (1, 1, 0), 1))):  # first terminal on ground: -(v(n3) i(R2))
        assert _power_factors(ckt, power(name)) == want, name
    for bad in ("R3", "R9", "r1b", "v(n1)", ""):  # both on ground, unknown, ambiguous (case-insensitive), not an element (2x)
        with pytest.raises(ValueError):
            _power_factors(ckt, power(bad))
    for a, b in (("v(n1)", "i(R9)"), ("v(nope)", "i(R1)"), ("v(n1", "i(R1)"), ("v(n1)", "R1"), ("i(R1,R2)", "v(n1)"), ("v(0,n1)", "i(R1)"), ("v(n1)", "i(r1b)")):
        with pytest.raises(ValueError):
            _power_factors(ckt, power(a, b))
    assert _power_factors(ckt, power("v(n1,n2)", "v(n3)")) == ((0, node("n1"), node("n2")), (0, node("n3"), 0), 0)
    assert _power_factors(ckt, power("i(L1)", "i(d1)")) == ((1, 6, 0), (1, 10, 0), 0)
    for args in ((1,), ("v(a)", 2), (None,)):
        with pytest.raises(TypeError):
            power(*args)
    with pytest.raises(TypeError):
        efficiency("R1", stats("v(n1)"))
    with pytest.raises(TypeError):
        measureTRAN(ckt, {"p": "R1"}, backend=PerInstanceOracle())
    e = efficiency("R1", power("v(n1)", "i(V1)", t_from=2e-6), t_to=9e-6)
    assert e == Efficiency(Power("R1"), Power("v(n1)", "i(V1)", 2e-6), None, 9e-6)
    assert e.parts() == [Power("R1", None, None, 9e-6), Power("v(n1)", "i(V1)", 2e-6, 9e-6)]  # (its window, where given, replaces the parts')
    # the plan's records: columns of the recorded nodes, the sign, the windows; currents are needed
    p = _Plan(ckt, {"r2": power("R2", t_from=3e-6), "e": e, "vv": power("v(n1,n2)", "v(n3)")}, 1e-6, 20)
    cols = {n: c for c, n in enumerate(p.out_nodes)}
    assert p.need_i and p.out_nodes == sorted([node("n1"), node("n2"), node("n3")])
    assert [tuple(q) for q in p.preqs] == [(0, cols[node("n3")], -1, 1, 1, -1, 1, 0, 3, 20), (0, cols[node("n3")], -1, 1, 0, -1, 0, 0, 0, 9),
                                           (0, cols[node("n1")], -1, 1, 7, -1, 0, 0, 2, 9), (0, cols[node("n1")], cols[node("n2")], 0, cols[node("n3")], -1, 0, 0, 0, 20)]
    assert [(n, k) for n, _, k in p.names] == [("r2", 0), ("e", 1), ("vv", 3)]
    assert not _Plan(ckt, {"vv": power("v(n1,n2)", "v(n3)")}, 1e-6, 20).need_i
    with pytest.raises(ValueError):
        _Plan(ckt, {"p": power("R1", t_from=9e-6, t_to=3e-6)}, 1e-6, 20)


def test_grounded_first_terminal_equals_the_general_form_written_by_hand(oracle_backend):
    got = measureTRAN(parseNetlist(ELEMENTS), {"el": power("R2"), "hand": power("v(n3)", "i(R2)"), "fwd": power("R1"), "fwd_hand": power("v(n3)", "i(R1)")},
                      backend=oracle_backend)
    el, hand = got["el"], got["hand"]
    assert got["fwd"] == got["fwd_hand"]
    # the exact negation: every linear field changes its sign and nothing else, the extremes change places
    for k in ("energy", "avg", "first", "final"):
        assert el[k] == -hand[k], k
    assert (el["peak"], el["t_peak"], el["min"], el["t_min"]) == (-hand["min"], hand["t_min"], -hand["peak"], hand["t_peak"])
    assert (el["rms_a"], el["rms_b"], el["apparent"]) == (hand["rms_a"], hand["rms_b"], hand["apparent"]) and el["pf"] == -hand["pf"]
    assert el["avg"] > 0 and got["fwd"]["avg"] > 0  # (a resistor absorbs, whichever way round it is wired)


def test_dc_divider_powers_and_efficiency(oracle_backend):
    got = measureTRAN(parseNetlist(DIVIDER), {"v1": power("V1"), "r1": power("R1"), "r2": power("R2"), "eff": efficiency("R2", "V1"),
                                              "eff2": efficiency(power("v(out)", "i(R2)"), power("V1"), t_from=2e-6)}, backend=oracle_backend)
    assert abs(got["v1"]["avg"] - -2.5e-4) <= BAR * 2.5e-4   # the source delivers: negative
    assert abs(got["r2"]["avg"] - 1.875e-4) <= BAR * 1.875e-4
    assert abs(got["r1"]["avg"] - 0.625e-4) <= BAR * 0.625e-4
    for k in ("eff", "eff2"):
        e = got[k]
        assert abs(e["eff"] - 0.75) <= BAR * 0.75 and abs(e["p_load"] - 1.875e-4) <= BAR * 1.875e-4 and abs(e["p_source"] - 2.5e-4) <= BAR * 2.5e-4
    for k in ("r1", "r2"):
        assert abs(got[k]["pf"] - 1.0) <= BAR and abs(got[k]["apparent"] - got[k]["avg"]) <= BAR * got[k]["avg"]
    assert abs(got["v1"]["pf"] - -1.0) <= BAR
    assert abs(got["r2"]["energy"] - 1.875e-4 * 10e-6) <= BAR * 1.875e-4 * 10e-6 and got["r2"]["t_peak"] <= 10e-6 and got["r2"]["first"] == got["r2"]["final"]


def test_resistor_energy_equals_the_trapezoid_of_simulateTRAN_s_waveforms(oracle_backend):
    tr = simulateTRAN(parseNetlist(RC), backend=oracle_backend, as_lists=False)
    v = tr["nodeVoltages"]["in"] - tr["nodeVoltages"]["out"]
    i = tr["elementCurrents"]["R1"]
    p = v * i
    n, dt = len(p), 1e-6
    assert n == 101
    got = measureTRAN(parseNetlist(RC), {"r1": power("R1"), "late": power("R1", t_from=30e-6, t_to=70e-6), "vi": power("v(in,out)", "i(R1)"),
                                         "c1": power("C1"), "v1": power("V1"), "s": stats("v(out)")}, backend=oracle_backend)
    assert got["r1"] == got["vi"]
    bound = (n + 1) * U * float(np.abs(p).sum()) * dt
    assert abs(got["r1"]["energy"] - float(trapz(p, dx=dt))) <= bound and got["r1"]["energy"] > 0
    assert abs(got["late"]["energy"] - float(trapz(p[30:71], dx=dt))) <= (41 + 1) * U * float(np.abs(p[30:71]).sum()) * dt
    assert abs(got["r1"]["avg"] - float(trapz(p, dx=dt)) / (100 * dt)) <= bound / (100 * dt) * (1 + 4 * U)
    k = int(np.argmax(p))
    assert (got["r1"]["peak"], got["r1"]["t_peak"], got["r1"]["min"], got["r1"]["first"], got["r1"]["final"]) == (p[k], k * dt, p.min(), p[0], p[-1])
    assert abs(got["r1"]["rms_a"] - math.sqrt(float(trapz(v * v, dx=dt)) / (100 * dt))) <= 1e-12 * got["r1"]["rms_a"]
    assert abs(got["r1"]["rms_b"] - math.sqrt(float(trapz(i * i, dx=dt)) / (100 * dt))) <= 1e-12 * got["r1"]["rms_b"]
    assert abs(got["r1"]["pf"] - 1.0) <= BAR and abs(got["c1"]["pf"]) < 0.9  # (a resistor's v and i are in proportion; a capacitor's are not)
    # what the source delivers goes into R1 and C1: Tellegen, to rounding
    assert abs(got["v1"]["energy"] + got["r1"]["energy"] + got["c1"]["energy"]) <= 1e-9 * got["r1"]["energy"]
    assert got["s"] == measureTRAN(parseNetlist(RC), {"s": stats("v(out)")}, backend=oracle_backend)["s"]


def test_one_sample_window_rules(oracle_backend):
    q = make_power_reqs([(0, 0, -1, 1, 0, -1, 0, 7, 7)])[0]
    row = np.array([-6.0, -6.0, 7, 7, -6.0, -6.0, -6.0, 4.0, 9.0, -2.0, -2.0, 3.0, 3.0, 0, 0, 0])
    assert derive_power(q, row, 1e-6) == {"energy": 0.0, "avg": -6.0, "peak": -6.0, "t_peak": 7e-6, "min": -6.0, "t_min": 7e-6, "first": -6.0, "final": -6.0,
                                          "rms_a": 2.0, "rms_b": 3.0, "apparent": 6.0, "pf": -1.0}
    zero = derive_power(q, np.zeros(16), 1e-6)
    assert zero["apparent"] == 0.0 and zero["pf"] is None and zero["avg"] == 0.0
    assert derive_efficiency([q, q], [row, np.zeros(16)], 1e-6) == {"p_load": -6.0, "p_source": -0.0, "eff": None}
    assert derive_efficiency([q, q], [np.abs(row), row], 1e-6) == {"p_load": 6.0, "p_source": 6.0, "eff": 1.0}
    got = measureTRAN(parseNetlist(DIVIDER), {"p": power("R2", t_from=4e-6, t_to=4e-6), "e": efficiency("R2", "V1", t_from=4e-6, t_to=4.2e-6)}, backend=oracle_backend)
    assert got["p"]["energy"] == 0.0 and got["p"]["avg"] == got["p"]["first"] == got["p"]["final"] == got["p"]["peak"] and got["p"]["t_peak"] == 4e-6
    assert abs(got["p"]["avg"] - 1.875e-4) <= BAR * 1.875e-4 and abs(got["p"]["rms_a"] - 0.75) <= BAR and abs(got["e"]["eff"] - 0.75) <= BAR


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
    base = golden_netlist(load_golden("boost_probe"))
    texts = [variant(base, k) for k in range(3)]
    m = {"sw": power("SM1"), "d": power("DD1"), "in": power("Vsimulation_voltage_source_0"), "eff": efficiency("RR1", "Vsimulation_voltage_source_0", t_from=0.05),
         "s": stats("v(n3)"), "w": when("v(n3)", 5.0)}
    batch, solo = [parseNetlist(t) for t in texts], [parseNetlist(t) for t in texts]
    be = _Oracle()
    got = measureTRANBatch(batch, m, backend=be)
    assert [n for n, _ in be.launches] == [3]
    for g, c, b in zip(got, solo, batch):
        assert g == measureTRAN(c, m, backend=_Oracle()) and _state(b) == _state(c)
        assert 0.0 < g["eff"]["eff"] <= 1.0 + BAR and g["in"]["avg"] < 0 and g["sw"]["avg"] >= 0 and g["d"]["avg"] >= 0


def test_a_dict_without_these_specs_takes_the_path_it_took():
    """The backend sees the call it saw before — never run_measure_power —, the result is the object it was, and the batch's
    grouping key is the one it was."""
    calls = []

    class Recorder(_Oracle):
        def _note(self, name, flat, steps, dt, src, lists):
            from spicey_amd.measure import reduce_reference, reduce_reference_fourier, reduce_reference_timing
            calls.append((name, [len(lst) for lst in lists]))
            res = self.run(flat, steps, dt, src)
            for key, fn, lst in zip(("meas", "four", "timing"), (reduce_reference, reduce_reference_fourier, reduce_reference_timing), lists):
                res[key] = fn(res["out_v"], res["out_i"], lst, dt)
            return res

        def run_measure(self, flat, steps, dt, src, reqs, want_iters=True):
            return self._note("run_measure", flat, steps, dt, src, (reqs,))

        def run_measure_fourier(self, flat, steps, dt, src, reqs, freqs, want_iters=True):
            return self._note("run_measure_fourier", flat, steps, dt, src, (reqs, freqs))

        def run_measure_timing(self, flat, steps, dt, src, reqs, freqs, treqs, want_iters=True):
            return self._note("run_measure_timing", flat, steps, dt, src, (reqs, freqs, treqs))

        def run_measure_power(self, *a, **k):
            raise AssertionError("a dict without power() / efficiency() reached the product pass")

    s, f, w = {"s": stats("v(out)"), "x": cross("v(out)", 0.5)}, {"f": fourier("v(out)", 1.0 / 40e-6, periods=2)}, {"w": when("v(out)", 0.5)}
    for m, want in ((s, ("run_measure", [2])), ({**s, **f}, ("run_measure_fourier", [2, 1])), ({**f, **w}, ("run_measure_timing", [0, 1, 1]))):
        calls.clear()
        got = measureTRAN(parseNetlist(RC), m, backend=Recorder())
        assert calls == [want] and got == measureTRAN(parseNetlist(RC), m, backend=_Oracle()) and list(got) == list(m)
    ckt = parseNetlist(RC)
    p = _Plan(ckt, {**s, **f, **w}, 1e-6, 100)
    assert len(p.preqs) == 0 and p.key() == p.reqs.tobytes() + b"|" + p.freqs.tobytes() + b"|" + p.treqs.tobytes()
    p = _Plan(ckt, {**s, **f}, 1e-6, 100)
    assert p.key() == p.reqs.tobytes() + b"|" + p.freqs.tobytes()
    q = _Plan(ckt, {**s, **f, "p": power("C1")}, 1e-6, 100)  # (v(out) i(C1): the recorded nodes stay the same)
    assert q.key() == p.key() + b"|p|" + q.preqs.tobytes()
    assert _Plan(ckt, {"p": power("R1")}, 1e-6, 100).key() != _Plan(ckt, {"p": power("C1")}, 1e-6, 100).key()
    # with the specs, a backend that has the method gets it, with all five lists
    seen = []

    class WithPower(_Oracle):
        def run_measure_power(self, flat, steps, dt, src, reqs, freqs, treqs, sreqs, preqs, want_iters=True):
            from spicey_amd.measure import backend_reduce
            seen.append([len(x) for x in (reqs, freqs, treqs, sreqs, preqs)])
            return backend_reduce(_Oracle(), flat, steps, dt, src, reqs, freqs, treqs, True, sreqs, preqs)

    got = measureTRAN(parseNetlist(RC), {**s, "e": efficiency("R1", "V1")}, backend=WithPower())
    assert seen == [[2, 0, 0, 0, 2]] and got == measureTRAN(parseNetlist(RC), {**s, "e": efficiency("R1", "V1")}, backend=_Oracle())
