"""fourier() through measureTRAN / measureTRANBatch on the CPU: the oracle is a backend without run_measure_fourier, so the
waveforms come from backend.run and the sums from reduce_reference_fourier.  Synthetic waveforms with known harmonics
must come back to 1e-12 of the largest amplitude; on a simulated circuit every value is recomputed here from
simulateTRAN's recorded waveform."""
import math
import subprocess

import numpy as np
import pytest

from batch_variants import PerInstanceOracle, variant
from conftest import REPO, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.measure import (cross, derive_fourier, fourier, fourier_window, make_four_reqs, measureTRAN, measureTRANBatch,
                                reduce_reference_fourier, stats)
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError, simulateTRAN

U = 2.0 ** -52
# a PULSE source whose period is 20 steps, into an RC
PULSE_RC = "* pulse into RC\nV1 in 0 PULSE(0 1 0 1u 1u 8u 20u)\nR1 in out 1k\nC1 out 0 2n\n.tran 1u 100u\n.end\n"


class _Oracle(PerInstanceOracle):
    """The per-instance oracle (it always computes the currents, and hands them out only when asked)."""

    def run(self, flat, steps, dt, src, want_currents=True, want_iters=True):
        res = super().run(flat, steps, dt, src, True, want_iters)
        if not want_currents:
            res["out_i"] = None
        return res


def _state(ckt):
    return ([c.vPrev for c in ckt.C], [l.iPrev for l in ckt.L], [d.vdPrev for d in ckt.D], [s.isOn for s in ckt.S])


def test_synthetic_harmonics_come_back():
    dt, f0 = 1e-6, 1.0 / (64 * 1e-6)
    n_points = 64 * 5 + 30
    amp = [0.0, 2.0, 0.0, 0.5, 0.25, 0.0, 1e-3, 0.125, 0.0, 0.3]   # A_1 .. A_9 behind A0
    ph = [0.0, 0.3, 0.0, -2.0, 3.0, 0.0, 1.0, -0.7, 0.0, 2.9]
    a0 = -0.75
    s = np.arange(n_points)
    x = a0 + sum(amp[h] * np.cos(2 * np.pi * h * f0 * s * dt + ph[h]) for h in range(1, 10))
    assert 9 * f0 * dt < 0.25  # (well under Nyquist)
    out_v = np.stack([x, 0.5 * x], axis=1)[None]
    amax = max(amp)
    for s0, s1 in ((23, 23 + 64 * 4), (64, 64 * 3), (7, 7 + 64)):  # whole periods, none starting at step 0
        reqs = make_four_reqs([(0, 0, -1, 9, s0, s1, f0), (0, 0, 1, 9, s0, s1, f0)])  # x, and x - x / 2
        rows = reduce_reference_fourier(out_v, None, reqs, dt)[0]
        for k, scale in ((0, 1.0), (1, 0.5)):
            d = derive_fourier(reqs[k], rows[k], dt)
            assert d["f0"] == f0 and abs(d["periods"] - (s1 - s0) / 64) < 1e-12
            assert abs(d["dc"] - scale * a0) <= 1e-12 * amax
            for h in range(1, 10):
                m, p = d["mag"][h - 1], math.radians(d["phase_deg"][h - 1])
                assert abs(m - scale * amp[h]) <= 1e-12 * amax, (s0, h, m)
                # (the phasor, so that a harmonic of no amplitude has no phase to miss)
                assert abs(m * complex(math.cos(p), math.sin(p)) - scale * amp[h] * complex(math.cos(ph[h]), math.sin(ph[h]))) <= 1e-12 * amax, (s0, h)
            thd = math.sqrt(sum(a * a for a in amp[2:])) / amp[1]
            assert abs(d["thd"] - thd) <= 1e-12 * amax / amp[1]
    one = derive_fourier(make_four_reqs([(0, 0, -1, 1, 64, 128, f0)])[0], reduce_reference_fourier(out_v, None, make_four_reqs([(0, 0, -1, 1, 64, 128, f0)]), dt)[0, 0], dt)
    assert one["thd"] is None and len(one["mag"]) == 1
    zero = derive_fourier(make_four_reqs([(0, 0, -1, 3, 64, 128, f0)])[0], np.zeros(7), dt)
    assert zero["thd"] is None and zero["mag"] == [0.0, 0.0, 0.0] and zero["dc"] == 0.0


def _recompute(x, s0, s1, f0, dt, H):
    """The harmonics of samples x[s0:s1] by numpy's own sums."""
    n = s1 - s0
    s = np.arange(s0, s1)
    out = {"dc": float(np.sum(x[s0:s1])) / n, "mag": [], "phase": []}
    for h in range(1, H + 1):
        a = 2.0 * float(np.sum(x[s0:s1] * np.cos(2 * np.pi * h * f0 * s * dt))) / n
        b = 2.0 * float(np.sum(x[s0:s1] * np.sin(2 * np.pi * h * f0 * s * dt))) / n
        out["mag"].append(math.hypot(a, b))
        out["phase"].append(math.degrees(math.atan2(-b, a)))
    return out


def test_pulse_into_rc_equals_the_recorded_waveform(oracle_backend):
    f0 = 1.0 / 20e-6
    ref = simulateTRAN(parseNetlist(PULSE_RC), backend=oracle_backend)
    x = np.array(ref["nodeVoltages"]["out"])
    xin = np.array(ref["nodeVoltages"]["in"])
    assert len(x) == 101
    m = {"f": fourier("v(out)", f0, periods=2), "s": stats("v(out)"), "d": fourier("v(in,out)", f0, harmonics=5, t_from=20e-6, t_to=80e-6),
         "i": fourier("i(R1)", f0, harmonics=3, periods=1, t_to=90e-6), "c": cross("v(out)", 0.5)}
    got = measureTRAN(parseNetlist(PULSE_RC), m, backend=oracle_backend)
    assert list(got) == list(m)
    plain = measureTRAN(parseNetlist(PULSE_RC), {"s": stats("v(out)"), "c": cross("v(out)", 0.5)}, backend=oracle_backend)
    assert got["s"] == plain["s"] and got["c"] == plain["c"]
    cur = np.array(ref["elementCurrents"]["R1"])
    for key, sig, s0, s1, H in (("f", x, 60, 100, 9), ("d", xin - x, 20, 80, 5), ("i", cur, 70, 90, 3)):
        g, e = got[key], _recompute(sig, s0, s1, f0, 1e-6, H)
        scale = float(np.max(np.abs(sig[s0:s1])))
        assert g["f0"] == f0 and abs(g["periods"] - (s1 - s0) / 20) < 1e-12 and len(g["mag"]) == H
        assert abs(g["dc"] - e["dc"]) <= 1e-12 * scale, key
        for h in range(H):
            assert abs(g["mag"][h] - e["mag"][h]) <= 1e-12 * scale, (key, h)
            if e["mag"][h] > 1e-6 * scale:
                assert abs(g["phase_deg"][h] - e["phase"][h]) <= 1e-6, (key, h)
        assert abs(g["thd"] - math.sqrt(sum(v * v for v in e["mag"][1:])) / e["mag"][0]) <= 1e-10, key
    assert got["f"]["mag"][0] > 0.1 and got["f"]["thd"] > 0.01  # (a square wave through an RC: a fundamental and harmonics)


def test_window_rules_and_host_errors(oracle_backend):
    dt, steps = 1e-6, 100
    f0 = 1.0 / 20e-6
    assert fourier_window(fourier("v(a)", f0), dt, steps) == (0, 100)
    assert fourier_window(fourier("v(a)", f0, periods=2), dt, steps) == (60, 100)
    assert fourier_window(fourier("v(a)", f0, periods=3, t_to=90.4e-6), dt, steps) == (30, 90)
    assert fourier_window(fourier("v(a)", f0, t_from=19.5e-6, t_to=60.49e-6), dt, steps) == (20, 60)  # (the nearest step, ties later)
    assert fourier_window(fourier("v(a)", 1.0 / 20.4e-6, periods=2), dt, steps) == (59, 100)  # round(40.8)
    assert fourier_window(fourier("v(a)", 1.0 / 20.4e-6, periods=1), dt, steps) == (80, 100)  # (within half a step of a period: taken)
    for bad in (dict(periods=6), dict(t_from=50e-6, t_to=50e-6), dict(t_from=60e-6, t_to=40e-6), dict(t_from=50e-6, t_to=60e-6),
                dict(t_from=81e-6)):  # before the run, empty, empty, half a period, a step short of one period
        with pytest.raises(ValueError):
            fourier_window(fourier("v(a)", f0, **bad), dt, steps)
    with pytest.raises(ValueError, match="Nyquist"):
        fourier_window(fourier("v(a)", f0, harmonics=11), dt, steps)  # 11 f0 = 550 kHz > 500 kHz
    fourier_window(fourier("v(a)", f0, harmonics=10), dt, steps)  # (at Nyquist: taken)
    for kw in (dict(harmonics=0), dict(harmonics=17), dict(harmonics=2.5), dict(periods=0), dict(periods=1.5), dict(periods=2, t_from=0.0)):
        with pytest.raises(ValueError):
            fourier("v(a)", f0, **kw)
    for f in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            fourier("v(a)", f)
    # through the front end: the same errors, before anything runs
    for spec in (fourier("v(out)", f0, periods=6), fourier("v(out)", f0, harmonics=11), fourier("v(out)", f0, t_from=90e-6), fourier("v(nope)", f0)):
        with pytest.raises(ValueError):
            measureTRAN(parseNetlist(PULSE_RC), {"f": spec}, backend=oracle_backend)
    with pytest.raises(TypeError):
        measureTRAN(parseNetlist(PULSE_RC), {"f": ("v(out)", f0)}, backend=oracle_backend)
    only = measureTRAN(parseNetlist(PULSE_RC), {"f": fourier("v(out)", f0, periods=2)}, backend=oracle_backend)  # (no stats or cross at all)
    both = measureTRAN(parseNetlist(PULSE_RC), {"s": stats("v(in)"), "f": fourier("v(out)", f0, periods=2)}, backend=oracle_backend)
    assert only["f"] == both["f"]
    # a window that is no whole number of periods leaks, and says so
    leak = measureTRAN(parseNetlist(PULSE_RC), {"f": fourier("v(out)", f0, t_from=55e-6)}, backend=oracle_backend)["f"]
    assert leak["periods"] == pytest.approx(2.25) and leak["mag"] != only["f"]["mag"]


def test_state_write_back_equals_simulateTRAN(oracle_backend):
    for text, spec in ((PULSE_RC, fourier("v(out)", 1.0 / 20e-6, periods=2)), (golden_netlist(load_golden("half_bridge")), fourier("v(out)", 20e3, periods=3))):
        a, b = parseNetlist(text), parseNetlist(text)
        for rnd in range(2):  # the second call continues from the state the first one wrote
            simulateTRAN(a, backend=oracle_backend)
            measureTRAN(b, {"f": spec}, backend=oracle_backend)
            assert _state(a) == _state(b), rnd


def test_batch_slots_equal_solo_calls_and_a_singular_circuit_in_its_slot():
    texts = [variant(PULSE_RC, k) for k in range(3)]
    texts.insert(1, "* no transient\nV1 in 0 DC 1\nR1 in out 1k\n.end\n")
    f0 = 1.0 / 20e-6
    m = {"f": fourier("v(out)", f0, periods=2), "s": stats("v(out)", t_from=10e-6), "g": fourier("v(in,out)", f0, harmonics=10, periods=2),
         "i": fourier("i(c1)", f0, harmonics=4), "x": cross("v(out)", 0.4, dir="either")}
    batch, solo = [parseNetlist(t) for t in texts], [parseNetlist(t) for t in texts]
    be = _Oracle()
    for rnd in range(2):
        got = measureTRANBatch(batch, m, backend=be)
        assert got[1] is None
        for i, (g, c) in enumerate(zip(got, solo)):
            if i != 1:
                assert g == measureTRAN(c, m, backend=_Oracle()), (rnd, i)
                assert _state(batch[i]) == _state(c), (rnd, i)
    assert [n for n, _ in be.launches] == [3, 3]  # one launch per call
    # circuits whose fourier tables differ (another f0 resolves to another window) do not share a launch
    be = _Oracle()
    measureTRANBatch([parseNetlist(texts[0]), parseNetlist(texts[0].replace(".tran 1u 100u", ".tran 1u 120u"))], {"f": fourier("v(out)", f0, periods=2)}, backend=be)
    assert [n for n, _ in be.launches] == [1, 1]
    # a singular instance inside a launch: near_sing_b's island grounded through 1e16 ohm next to solvable variants
    nsb = golden_netlist(load_golden("near_sing_b"))
    isl = [nsb.replace("1e16", "1k"), nsb, nsb.replace("1e16", "2k")]
    m = {"s": stats("v(a)"), "f": fourier("v(a)", 250e3, harmonics=1, periods=1)}
    ck = [parseNetlist(t) for t in isl]
    before = _state(ck[1])
    be = _Oracle()
    got = measureTRANBatch(ck, m, backend=be)
    assert be.launches[0][0] == 3
    assert isinstance(got[1], SingularMatrixError) and str(got[1]) == "Singular matrix (real)" and _state(ck[1]) == before
    for i in (0, 2):
        assert got[i] == measureTRAN(parseNetlist(isl[i]), m, backend=_Oracle())
        assert got[i]["f"]["dc"] == 1.0 and got[i]["f"]["periods"] == 1.0
    with pytest.raises(SingularMatrixError):
        measureTRAN(parseNetlist(nsb), m, backend=_Oracle())


def test_four_req_dtype_is_the_compilers_layout(tmp_path):
    fields = list(abi.FOUR_REQ_DTYPE.names)
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{REPO}/include/spicey_hip.h"', "int main(void){"]
    src += [f'  printf("{f} %zu\\n", offsetof(SpiceyFourReq, {f}));' for f in fields]
    src += ['  printf("__size %zu\\n", sizeof(SpiceyFourReq));', '  printf("__max %d\\n", SPICEY_FOUR_MAX_HARM);', "  return 0; }"]
    c = tmp_path / "four_req.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "four_req"
    subprocess.run(["gcc", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert got.pop("__size") == abi.FOUR_REQ_DTYPE.itemsize == 40 and got.pop("__max") == abi.FOUR_MAX_HARM
    assert got == {f: abi.FOUR_REQ_DTYPE.fields[f][1] for f in fields}
    import ctypes
    assert {f: getattr(abi.SpiceyFourReq, f).offset for f in fields} == got and ctypes.sizeof(abi.SpiceyFourReq) == 40
