"""spectrum() and dominant() through measureTRAN / measureTRANBatch on the CPU: the oracle is a backend without
run_measure_spectrum, so the waveforms come from backend.run and the transform from reduce_reference_spectrum.  A square
wave's fundamental must land on its bin; the window and band rules; on golden circuits every derived value is recomputed
here from the recorded waveforms."""
import math

import numpy as np
import pytest

from batch_variants import PerInstanceOracle, variant
from conftest import farr, golden_netlist, load_golden
from spicey_amd import abi
from spicey_amd.measure import (cross, derive_spectrum, dominant, fourier, make_spec_reqs, measureTRAN, measureTRANBatch, reduce_reference_spectrum,
                                spectrum, spectrum_window, stats, when)
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError, simulateTRAN

# a square wave of period 64 us into an RC: the last 1024 samples of the run hold 16 periods (to 0.1 %)
SQUARE_RC = "* square wave into RC\nV1 in 0 PULSE(0 1 0 1n 1n 32u 64u)\nR1 in out 1k\nC1 out 0 1n\n.tran 1u 1023u\n.end\n"


class _Oracle(PerInstanceOracle):
    """The per-instance oracle (it always computes the currents, and hands them out only when asked)."""

    def run(self, flat, steps, dt, src, want_currents=True, want_iters=True):
        res = super().run(flat, steps, dt, src, True, want_iters)
        if not want_currents:
            res["out_i"] = None
        return res


def _state(ckt):
    return ([c.vPrev for c in ckt.C], [l.iPrev for l in ckt.L], [d.vdPrev for d in ckt.D], [s.isOn for s in ckt.S])


def test_square_wave_has_its_fundamental_on_bin_16(oracle_backend):
    ckt = parseNetlist(SQUARE_RC)
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    assert steps + 1 >= 1024
    df = 1.0 / (1024 * dt)
    got = measureTRAN(ckt, {"d": dominant("v(out)", n=1024), "s": spectrum("v(in)", n=1024, window="rect")}, backend=oracle_backend)
    d, s = got["d"], got["s"]
    assert d["bin"] == 16 and d["freq_bin"] == 16 * df and d["n"] == 1024 and d["df"] == df
    assert abs(d["freq"] - 16 * df) < 0.1 * df and 0.3 < d["mag"] < 2 / math.pi * 1.01  # (the fundamental of a 0..1 square wave, behind an RC)
    assert s["n"] == 1024 and s["window"] == "rect" and len(s["freq"]) == len(s["mag"]) == len(s["phase_deg"]) == 513 and s["freq"][16] == 16 * df
    assert s["mag"][16] > s["mag"][15] and s["mag"][16] > s["mag"][17]
    assert 0.55 < s["mag"][16] < 2 / math.pi * 1.01 and abs(s["mag"][0] - 0.5) < 1e-2  # the fundamental 2 / pi (less a little leakage) and the mean


def test_window_and_band_rules_and_their_errors(oracle_backend):
    dt, steps = 1e-6, 1023
    assert spectrum_window(spectrum("v(a)"), dt, steps) == (0, 10, 0, 512)
    assert spectrum_window(dominant("v(a)"), dt, steps) == (0, 10, 1, 512)  # (DC excluded)
    assert spectrum_window(spectrum("v(a)", n=256), dt, steps) == (768, 8, 0, 128)  # the LAST n samples of the window
    assert spectrum_window(spectrum("v(a)", n=256, t_to=511.4e-6), dt, steps) == (256, 8, 0, 128)
    assert spectrum_window(spectrum("v(a)", t_from=100e-6, t_to=400.5e-6), dt, steps) == (146, 8, 0, 128)  # 302 samples (a tie goes later) -> 256
    assert spectrum_window(spectrum("v(a)", t_from=100e-6, t_to=107e-6), dt, steps) == (100, 3, 0, 4)
    assert spectrum_window(spectrum("v(a)"), dt, 20000) == (20001 - 8192, 13, 0, 4096)  # capped at 8192
    # bands: ceil / floor of f N dt, clamped to [0, N/2]
    df = 1.0 / (1024 * dt)
    assert spectrum_window(spectrum("v(a)", f_from=2.5 * df, f_to=7.5 * df), dt, steps)[2:] == (3, 7)
    assert spectrum_window(spectrum("v(a)", f_from=0.0, f_to=1e9), dt, steps)[2:] == (0, 512)
    assert spectrum_window(dominant("v(a)", f_from=0.0), dt, steps)[2:] == (0, 512)
    assert spectrum_window(dominant("v(a)", f_from=100e3, f_to=5e6), dt, steps)[2:] == (103, 512)
    assert spectrum_window(spectrum("v(a)", n=8, f_from=499e3), dt, steps)[2:] == (4, 4)
    for spec in (spectrum("v(a)", f_from=2.2 * df, f_to=2.8 * df), spectrum("v(a)", f_from=600e3), spectrum("v(a)", f_from=3 * df, f_to=2 * df),
                 spectrum("v(a)", n=2048), spectrum("v(a)", n=256, t_from=900e-6), spectrum("v(a)", t_from=100e-6, t_to=106e-6),
                 spectrum("v(a)", t_from=300e-6, t_to=200e-6)):  # no bin in the band (3x); longer than the run / the window; under 8 samples; empty
        with pytest.raises(ValueError):
            spectrum_window(spec, dt, steps)
    for kw in (dict(n=0), dict(n=4), dict(n=100), dict(n=16384), dict(n=64.5), dict(n=True), dict(window="hamming"), dict(window=1),
               dict(f_from=-1.0), dict(f_to=float("nan")), dict(f_from=float("inf"))):
        for make in (spectrum, dominant):
            with pytest.raises(ValueError):
                make("v(a)", **kw)
    # through the front end: the same errors, before anything runs
    for spec in (spectrum("v(out)", n=2048), dominant("v(out)", f_from=600e3), spectrum("v(nope)")):
        with pytest.raises(ValueError):
            measureTRAN(parseNetlist(SQUARE_RC), {"s": spec}, backend=oracle_backend)
    only = measureTRAN(parseNetlist(SQUARE_RC), {"d": dominant("v(out)", n=64)}, backend=oracle_backend)  # (no other family at all)
    both = measureTRAN(parseNetlist(SQUARE_RC), {"s": stats("v(in)"), "d": dominant("v(out)", n=64)}, backend=oracle_backend)
    assert only["d"] == both["d"] and only["d"]["bin"] == 1


def _recompute_spectrum(x, N, window, b0, b1, dt):
    """spectrum()'s values from the last N samples of x by numpy's own FFT."""
    y = x[len(x) - N:]
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N) if window == "hann" else np.ones(N)
    X = np.fft.rfft(y * w)
    side = np.where((np.arange(N // 2 + 1) == 0) | (np.arange(N // 2 + 1) == N // 2), 1.0, 2.0)
    return (np.arange(N // 2 + 1) / (N * dt))[b0:b1 + 1], (np.abs(X) * side / w.sum())[b0:b1 + 1], np.degrees(np.angle(X))[b0:b1 + 1]


def test_derived_values_equal_those_of_the_recorded_golden_waveforms(oracle_backend):
    g = load_golden("lc_tank")
    run = g["runs"][0]
    ckt = parseNetlist(golden_netlist(g))
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    vc, vb, il = farr(run["V"]["c"]), farr(run["V"]["b"]), farr(run["I"]["L2"])
    assert len(vc) == steps + 1 == 201
    m = {"ring": dominant("v(c)"), "full": spectrum("v(c)", window="rect"), "hann": spectrum("v(b,c)", n=64, f_from=20e3, f_to=200e3),
         "cur": spectrum("i(L2)", n=128, t_to=150e-6), "dc": dominant("v(c)", f_from=0.0, n=32), "s": stats("v(c)"), "x": cross("v(c)", 1.0)}
    got = measureTRAN(ckt, m, backend=oracle_backend)
    assert list(got) == list(m)
    plain = measureTRAN(parseNetlist(golden_netlist(g)), {"s": stats("v(c)"), "x": cross("v(c)", 1.0)}, backend=oracle_backend)
    assert got["s"] == plain["s"] and got["x"] == plain["x"]
    for key, x, N, window, b0, b1 in (("full", vc, 128, "rect", 0, 64), ("hann", vb - vc, 64, "hann", 2, 12), ("cur", il[:151], 128, "hann", 0, 64)):
        f, mag, ph = _recompute_spectrum(x, N, window, b0, b1, dt)
        s = got[key]
        scale = float(np.max(np.abs(x[len(x) - N:])))
        assert s["n"] == N and s["df"] == 1.0 / (N * dt) and s["window"] == window and len(s["mag"]) == b1 - b0 + 1
        assert np.allclose(s["freq"], f, rtol=1e-15, atol=0) and np.abs(np.array(s["mag"]) - mag).max() <= 1e-12 * scale, key
        for k in range(len(mag)):
            if mag[k] > 1e-6 * scale:
                assert abs((s["phase_deg"][k] - ph[k] + 180.0) % 360.0 - 180.0) <= 1e-6, (key, k)
    # the dominant bin: numpy's argmax of the Hann spectrum (without DC by default), refined by the parabola through its neighbours
    for key, N, lo in (("ring", 128, 1), ("dc", 32, 0)):
        _, mag, _ = _recompute_spectrum(vc, N, "hann", 0, N // 2, dt)
        side = np.where((np.arange(N // 2 + 1) == 0) | (np.arange(N // 2 + 1) == N // 2), 1.0, 2.0)
        amp = mag / side  # |X_k| / sum(w): the device compares powers, not the one-sided magnitudes
        k = lo + int(np.argmax(amp[lo:]))
        d = got[key]
        df = 1.0 / (N * dt)
        assert d["bin"] == k and d["freq_bin"] == k * df and d["n"] == N and d["df"] == df and abs(d["mag"] - mag[k]) <= 1e-12 * mag[k]
        delta = 0.5 * (amp[k - 1] - amp[k + 1]) / (amp[k - 1] - 2 * amp[k] + amp[k + 1]) if 1 <= k < N // 2 else 0.0
        assert abs(d["freq"] - (k + delta) * df) <= 1e-9 * df  # (no clamp: beside the large DC bin the parabola leans far towards it)
    assert got["dc"]["bin"] == 0 and got["dc"]["freq"] == 0.0  # (a missing neighbour: no refinement)
    # derive_spectrum on rows of its own: nothing wins -> every field None; a missing neighbour or a flat top -> delta = 0
    q = make_spec_reqs([(0, 0, -1, 1, 0, 4, 1, 0, 8)])[0]
    assert derive_spectrum(q, np.array([-1.0, 0, 0, 0, 0, 0, 0, 0]), 1e-6) == {k: None for k in ("bin", "freq", "mag", "freq_bin", "n", "df")}
    flat_top = derive_spectrum(q, np.array([3.0, 2.0, 0.0, 4.0, 4.0, 4.0, 0, 0]), 1e-6)
    assert flat_top["freq"] == flat_top["freq_bin"] == 3 / 16e-6 and flat_top["mag"] == 2.0 * 2.0 / 8.0
    assert derive_spectrum(q, np.array([8.0, 2.0, 0.0, 1.0, 4.0, -1.0, 0, 0]), 1e-6)["freq"] == 8 / 16e-6
    # the reference is what the API ran: one request by hand
    row = reduce_reference_spectrum(vc[None, :, None], None, make_spec_reqs([(0, 0, -1, 0, 201 - 128, 7, 0, 0, 64)]), dt)[0, 0]
    assert derive_spectrum(make_spec_reqs([(0, 0, -1, 0, 201 - 128, 7, 0, 0, 64)])[0], row, dt) == got["full"]


def test_state_write_back_equals_simulateTRAN(oracle_backend):
    for text, spec in ((SQUARE_RC, dominant("v(out)", n=256)), (golden_netlist(load_golden("half_bridge")), spectrum("v(out)", f_from=100e3, f_to=5e6))):
        a, b = parseNetlist(text), parseNetlist(text)
        for rnd in range(2):  # the second call continues from the state the first one wrote
            simulateTRAN(a, backend=oracle_backend)
            measureTRAN(b, {"f": spec}, backend=oracle_backend)
            assert _state(a) == _state(b), rnd


def test_batch_slots_equal_solo_calls_and_a_singular_circuit_in_its_slot():
    short = SQUARE_RC.replace(".tran 1u 1023u", ".tran 1u 130u")
    texts = [variant(short, k) for k in range(3)]
    texts.insert(1, "* no transient\nV1 in 0 DC 1\nR1 in out 1k\n.end\n")
    m = {"d": dominant("v(out)"), "s": stats("v(out)", t_from=10e-6), "g": spectrum("v(in,out)", n=64, window="rect"),
         "i": spectrum("i(c1)", n=32, f_to=200e3), "x": cross("v(out)", 0.4, dir="either"), "f": fourier("v(out)", 1.0 / 64e-6, periods=2),
         "w": when("v(out)", 0.5)}
    batch, solo = [parseNetlist(t) for t in texts], [parseNetlist(t) for t in texts]
    be = _Oracle()
    for rnd in range(2):
        got = measureTRANBatch(batch, m, backend=be)
        assert got[1] is None
        for i, (g, c) in enumerate(zip(got, solo)):
            if i != 1:
                assert g == measureTRAN(c, m, backend=_Oracle()), (rnd, i)
                assert _state(batch[i]) == _state(c), (rnd, i)
                assert g["d"]["n"] == 128 and g["d"]["bin"] == 2 and len(g["g"]["mag"]) == 33
    assert [n for n, _ in be.launches] == [3, 3]  # one launch per call
    # circuits whose spectrum tables differ (another run length resolves to another first step) do not share a launch
    be = _Oracle()
    measureTRANBatch([parseNetlist(texts[0]), parseNetlist(texts[0].replace(".tran 1u 130u", ".tran 1u 140u"))], {"d": dominant("v(out)", n=64)}, backend=be)
    assert [n for n, _ in be.launches] == [1, 1]
    # a singular instance inside a launch: near_sing_b's island grounded through 1e16 ohm next to solvable variants
    nsb = golden_netlist(load_golden("near_sing_b")).replace(".tran 1u 5u", ".tran 1u 9u")  # (10 samples: room for n = 8)
    assert ".tran 1u 9u" in nsb
    isl = [nsb.replace("1e16", "1k"), nsb, nsb.replace("1e16", "2k")]
    m = {"s": stats("v(a)"), "d": dominant("v(a)", n=8, f_from=0.0, window="rect")}
    ck = [parseNetlist(t) for t in isl]
    before = _state(ck[1])
    be = _Oracle()
    got = measureTRANBatch(ck, m, backend=be)
    assert be.launches[0][0] == 3
    assert isinstance(got[1], SingularMatrixError) and str(got[1]) == "Singular matrix (real)" and _state(ck[1]) == before
    for i in (0, 2):
        assert got[i] == measureTRAN(parseNetlist(isl[i]), m, backend=_Oracle())
        assert got[i]["d"]["bin"] == 0 and got[i]["d"]["mag"] == 1.0  # (v(a) = 1, as fourier's dc of the same circuit)
    with pytest.raises(SingularMatrixError):
        measureTRAN(parseNetlist(nsb), m, backend=_Oracle())


def test_a_dict_without_these_specs_takes_the_path_it_took():
    """The backend sees the call it saw before: run_measure / run_measure_fourier / run_measure_timing with their argument
    lists, never run_measure_spectrum; and the batch's grouping key is the one it was."""
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

        def run_measure_spectrum(self, *a, **k):
            raise AssertionError("a dict without spectrum() / dominant() reached the spectrum pass")

    s, f, w = {"s": stats("v(out)")}, {"f": fourier("v(out)", 1.0 / 64e-6, periods=2)}, {"w": when("v(out)", 0.5)}
    for m, want in ((s, ("run_measure", [1])), ({**s, **f}, ("run_measure_fourier", [1, 1])), ({**f, **w}, ("run_measure_timing", [0, 1, 1]))):
        calls.clear()
        got = measureTRAN(parseNetlist(SQUARE_RC), m, backend=Recorder())
        assert calls == [want] and got == measureTRAN(parseNetlist(SQUARE_RC), m, backend=_Oracle())
    from spicey_amd.measure import _Plan
    ckt = parseNetlist(SQUARE_RC)
    p = _Plan(ckt, {**s, **f, **w}, 1e-6, 1023)
    assert len(p.sreqs) == 0 and p.key() == p.reqs.tobytes() + b"|" + p.freqs.tobytes() + b"|" + p.treqs.tobytes()
    p = _Plan(ckt, {**s, **f}, 1e-6, 1023)
    assert p.key() == p.reqs.tobytes() + b"|" + p.freqs.tobytes()
    assert _Plan(ckt, {**s, "d": dominant("v(out)")}, 1e-6, 1023).key() != _Plan(ckt, {**s, "d": dominant("v(out)", n=512)}, 1e-6, 1023).key()
