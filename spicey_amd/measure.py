"""measureTRAN() / measureTRANBatch(): a few numbers per circuit instead of every sample (what SPICE calls .meas).

simulateTRAN returns whole waveforms; a sweep is usually run for the peak of an output, its ripple, an average current,
the first time a node crosses a threshold, the period of an oscillator.  Here the transient's waveforms stay on the
device and a reduction pass (spicey_run_measure, include/spicey_hip.h) brings back 8 doubles per (circuit, measure).  Only
the measured nodes are recorded (SpiceyDesc.out_nodes; .PRINT cards are ignored) and element currents only if a measure
names one.

Specs
    stats("v(out)")                        min, max, pp, t_min, t_max, first, final, integ, avg, rms
    cross("v(a,b)", 2.5, dir="rise")       count, t_first, t_last, freq
    fourier("v(out)", 50e3, harmonics=9)   f0, periods, dc, mag[], phase_deg[], thd   (see "Harmonics" below)
`signal` is "v(a)", "v(a,b)" (= v(a) - v(b), one rounded subtraction per sample; v(a,0) is v(a)) or "i(R1)" (the element
current simulateTRAN records under that name).  Node names resolve case-insensitively like the parser's; element names
too, and a name that several elements share is an error.

Windows.  t_from / t_to (seconds, None = the run's first / last point) select the inclusive window of steps
floor(t / dt + 0.5) — the nearest step, a tie going to the later one — clamped to [0, steps]; dt is the run's effective
step (abi.computeEffectiveTimeStep).

Derived values (on the host, from the device's {min, max, step_min, step_max, sum, sumsq, first, last}; n = samples in
the window): pp = max - min, t_min / t_max = step * dt (first occurrence), integ = dt (sum - (first + last) / 2) — the
trapezoidal rule on the uniform grid —, avg = integ / ((n - 1) dt), rms = sqrt(dt (sumsq - (first^2 + last^2) / 2) /
((n - 1) dt)); a one-sample window gives integ = 0, avg = first, rms = |first|.  Crossings: rise is x_k < level <=
x_k+1, fall x_k > level >= x_k+1, at linearly interpolated times; freq = (count - 1) / (t_last - t_first) for count >=
2, else None; t_first / t_last are None without a crossing.

Harmonics.  fourier(signal, f0, harmonics=9, t_from=None, t_to=None, periods=None) is what SPICE calls .four: the device
(spicey_run_measure_fourier, a second reduction behind the first over the same waveforms) sums C0 = sum x_s, C_h = sum x_s
cos(2 pi h f0 s dt), S_h = sum x_s sin(2 pi h f0 s dt) for h = 1..harmonics over the N samples step_from .. step_to - 1 —
the sample at step_to closes the last period and is left out (the rectangular rule, exact for a waveform periodic in the
window) — with s the ABSOLUTE step, so phases refer to t = 0.  The window is t_from / t_to by the rule above, or, with
periods=n, the last n periods that end at t_to: step_from = step_to - round(n / (f0 dt)).  On the host: dc = C0 / N, a_h =
2 C_h / N, b_h = 2 S_h / N, mag[h-1] = hypot(a_h, b_h), phase_deg[h-1] = degrees(atan2(-b_h, a_h)) — x(t) = M cos(2 pi h f0
t + phi) gives back M and phi —, thd = sqrt(sum_{h>=2} mag_h^2) / mag_1 (None when mag_1 == 0 or harmonics == 1), and
`periods` = N dt f0 as a float: a window that is no whole number of periods LEAKS (every harmonic picks up some of the
others); that is reported by this number and not refused.  ValueError for a window that is empty, reaches before the run
or is more than half a step shorter than one period, for harmonics outside 1..16 or above Nyquist (harmonics f0 > 1 / (2
dt)), and for periods= together with t_from=.  A dict without a fourier spec takes the path it always took.

Edge timing.  A third family, reduced on the device by a pass of its own (spicey_run_measure_timing, behind the other two
over the same waveforms; include/spicey_hip.h has the definition):
    when("v(out)", 2.5, dir="rise", n=1)                         t, level, count
    delay(trig=edge("v(g)", rel(0.5)), targ=edge("v(sw)", rel(0.5)))   t_trig, t_targ, delay, level_trig, level_targ,
                                                                 count_trig, count_targ
    rise_time("v(out)", lo=0.1, hi=0.9) / fall_time(...)         t_start, t_end, time, level_start, level_end
    settle("v(out)", tol=0.02)                                   t, level_lo, level_hi
A level is a number or rel(frac, of="minmax" | "ends", t_from=None, t_to=None): lo + frac * (hi - lo) with (lo, hi) the
signal's (min, max) or (first, last) sample over the base window (default: the whole run) of EACH circuit — a batch of
supply-scaled variants stays one launch.  n >= 1 is the n-th crossing of the window, n <= -1 the |n|-th from its end; dir
is "rise", "fall" or "either"; crossings and their interpolated times are cross()'s.  delay() searches the trig in the
window [t_from, t_to] and the targ from the trigger's own interval on (after_trig=True; a targ crossing in that interval
counts even if its interpolated time is a fraction of a step earlier, so the delay of two edges inside one step may be
slightly negative) or, with after_trig=False, in the whole window like SPICE's .meas trig/targ — a period is delay(trig=
edge(s, L, n=1), targ=edge(s, L, n=2), after_trig=False); with after_trig=True the same edge as trig and targ with n=1
finds the trigger's own crossing.  t / delay / time are None when an edge is not found; count is the number of crossings
in the edge's search range.  rise_time is the delay from the first rise through rel(lo) to the first rise through rel(hi)
at or after it (fall_time: falls through hi, then lo); settle is the later of the last crossings (either direction) of
rel(1 - tol, of="ends") and rel(1 + tol, of="ends"), 0.0 if the signal never leaves that band.  A window needs two steps.

Spectrum.  A fourth family, for the questions fourier() cannot answer because nobody knows f0 (what SPICE calls fft / spec):
a batched FFT on the device (spicey_run_measure_spectrum, a pass behind the other three over the same waveforms;
include/spicey_hip.h has the definition, bit for bit):
    spectrum("v(out)", n=None, window="hann", f_from=None, f_to=None)   n, df, window, freq[], mag[], phase_deg[]
    dominant("v(out)", n=None, window="hann", f_from=None, f_to=None)   bin, freq, mag, freq_bin, n, df
The N = n samples are the LAST n of the window [t_from, t_to] (the nearest-step rule above); n=None picks the largest power
of two that fits, at most 8192; n must be a power of two in 8..8192 and no longer than the window.  window is "hann" (the
periodic Hann window) or "rect".  df = 1 / (N dt), freq[k] = k df.  f_from / f_to select the bins ceil(f_from N dt) ..
floor(f_to N dt), clamped to [0, N/2] (default: all of them; dominant() starts at bin 1, so DC is excluded); an empty band
is a ValueError.  mag = |X_k| s / sum(w) with s = 1 for k = 0 and k = N/2, else 2 — a sine of amplitude A on a bin shows as
A — and phase_deg = degrees(atan2(im, re)) of X_k = sum_j x_j w_j exp(-2 pi i j k / N): the phase of a cosine, referred to
the window's FIRST sample (fourier() refers its phases to t = 0).  dominant() is the band's bin with the largest power (the
first of equals), found on the device; freq_bin = k df, and freq = (k + d) df refines it by the parabola through the
magnitudes a, b, c of the bins k-1, k, k+1: d = 0.5 (a - c) / (a - 2 b + c), d = 0 where a neighbour does not exist or the
denominator is 0.  Every field of dominant() is None when no bin has any power.  A dict without these specs takes the path
it always took.

Products.  A fifth family, the only one with two factors: the power an element takes, the power a supply delivers, an
efficiency, a power factor — v i formed sample by sample on the device (spicey_run_measure_power, a pass behind the other
four over the same waveforms; include/spicey_hip.h has the definition), because the average of a product is not the product
of the averages:
    power("R1")                             energy, avg, peak, t_peak, min, t_min, first, final, rms_a, rms_b, apparent, pf
    power("v(out)", "i(Rload)")             the same for any two signals (v v and i i too)
    efficiency("Rload", "V1")               p_load, p_source, eff
power(name) is the element form: the power the element ABSORBS under the passive sign convention, v(n1,n2) i(name) with the
element's own terminals (n1 / n2; nPlus / nMinus for a diode) and its recorded current, which flows from the first terminal
to the second.  A first terminal on ground gives -(v(n2) i(name)), an exact negation on the device; an element between
ground and ground is a ValueError; the name resolves as i(name) does.  A source that delivers power shows a negative avg
(i(V1) is the MNA branch current).  On the host, from the device's {min_p, max_p, step_min, step_max, sum_p, first_p, last_p,
sum_aa, sum_bb, first_a, last_a, first_b, last_b} with n the samples of the window: energy = dt (sum_p - (first_p + last_p) /
2) — the trapezoidal rule, as stats' integ —, avg = energy / ((n - 1) dt), peak = max_p at t_peak, min at t_min (first
occurrence), first, final, rms_a / rms_b by stats' trapezoid of squares, apparent = rms_a rms_b, pf = avg / apparent (None
when apparent == 0); a one-sample window gives energy = 0, avg = first, rms_a = |first_a|, rms_b = |first_b|.  efficiency(load,
source) takes element names or power(...) specs, goes down as two product requests and gives p_load = avg(load), p_source =
-avg(source), eff = p_load / p_source (None when p_source == 0); its t_from / t_to, where given, replace the parts' own.  A
dict without these specs takes the path it always took.

Values.  A sixth family, whose answers are samples of a waveform and not sums over it (the values pass of
spicey_run_reduced, behind the other five over the same waveforms; include/spicey_hip.h has the definition, bit for bit):
    trace("v(out)", buckets=512)            buckets, t_first[], first[], t_min[], min[], t_max[], max[], t_last[], last[], t[], v[]
    sample("v(out)", times)                 t[], value[], slope[]
    find("i(L1)", when=edge("v(sw)", 6.0, "fall"))   t, value, slope, level, count
    find("v(out)", at=1e-3) / deriv(...)    the same; deriv returns the slope as `value`
trace() is the decimation a line chart needs: the window [t_from, t_to] (the nearest-step rule above) of n samples is cut
into `buckets` buckets — bucket b holds the steps s0 + floor(b n / B) .. s0 + floor((b + 1) n / B) - 1 — and each gives its
first, last, minimum and maximum sample with their times (step * dt; of equal extremes the first), so no spike is lost and
the envelope is exact.  buckets above n is lowered to n (the waveform itself comes back); above abi.TRACE_MAX_BUCKETS after
that it is a ValueError.  t[] / v[] is the polyline to plot: per bucket its four points in step order, points of equal step
dropped, at most 4 B points.  sample() interpolates linearly at the given times: on the host q = t / dt (one division), k =
min(floor(q), steps - 1), f = q - k; on the device d = y[k+1] - y[k], value = y[k] + f d (y[k] for f = 0, y[k+1] for f = 1),
slope = d / dt.  A q less than half a step outside [0, steps] is clamped to that end (t[] reports the clamped time), further
out is a ValueError.  find(signal, when=edge(...)) is .meas FIND ... WHEN: the edge is found per circuit by the timing pass
(one hidden when() request in [t_from, t_to]; rel() levels work), and the signal is interpolated at that crossing's own k
and f = (L - x[k]) / (x[k+1] - x[k]); t = (k + f) dt is when()'s t bit for bit; t, value and slope are None when the edge is
not found; level and count are when()'s.  find(signal, at=t) is one sample() point (level and count None).  A run needs
two points for sample() and find().  A dict without these specs takes the path it always took.

reduce_reference() is the same definition in plain numpy; it is what the tests compare the device with, and what runs
behind a backend that has no run_measure (backend.run, then reduce_reference: the CPU oracle works unchanged);
reduce_reference_fourier() is the same for the harmonics, reduce_reference_timing() for the edge timing,
reduce_reference_spectrum() for the spectrum (that one bit for bit: the same elementwise operations in the same order),
reduce_reference_power() for the products (its sums in plain step order, every other field bit for bit),
reduce_reference_values() for the values (bit for bit: no field is a sum).
"""
from __future__ import annotations

import functools
import math
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .batch import group_launches, run_launch, write_state
from .netlist import ParsedCircuit
from .simulate import SingularMatrixError

_DIRS = {"rise": 1, "fall": -1, "either": 0}


@dataclass(frozen=True)
class Stats:
    signal: str
    t_from: Optional[float] = None
    t_to: Optional[float] = None


@dataclass(frozen=True)
class Cross:
    signal: str
    level: float
    dir: int = 1
    t_from: Optional[float] = None
    t_to: Optional[float] = None


@dataclass(frozen=True)
class Fourier:
    signal: str
    f0: float
    harmonics: int = 9
    t_from: Optional[float] = None
    t_to: Optional[float] = None
    periods: Optional[int] = None


_WINDOWS = {"rect": abi.SPEC_RECT, "hann": abi.SPEC_HANN}
_WINDOW_NAMES = {v: k for k, v in _WINDOWS.items()}


@dataclass(frozen=True)
class Spectrum:
    signal: str
    n: Optional[int] = None
    window: int = abi.SPEC_HANN
    f_from: Optional[float] = None
    f_to: Optional[float] = None
    t_from: Optional[float] = None
    t_to: Optional[float] = None
    kind: int = abi.SPEC_BINS


@dataclass(frozen=True)
class Power:
    a: str  # the element's name when b is None (the element form), else the first factor's signal
    b: Optional[str] = None
    t_from: Optional[float] = None
    t_to: Optional[float] = None

    def parts(self):
        return [self]


@dataclass(frozen=True)
class Efficiency:
    load: Power
    source: Power
    t_from: Optional[float] = None
    t_to: Optional[float] = None

    def parts(self):
        """The two product requests: load, source, under this spec's window where it gives one."""
        return [Power(p.a, p.b, p.t_from if self.t_from is None else self.t_from, p.t_to if self.t_to is None else self.t_to)
                for p in (self.load, self.source)]


_PRODUCTS = (Power, Efficiency)


@dataclass(frozen=True)
class Trace:
    signal: str
    buckets: int = 512
    t_from: Optional[float] = None
    t_to: Optional[float] = None


@dataclass(frozen=True)
class Sample:
    signal: str
    times: Tuple[float, ...]


@dataclass(frozen=True)
class Find:
    signal: str
    when: Optional["Edge"] = None  # the edge whose crossing is looked up, or
    at: Optional[float] = None     # a time
    t_from: Optional[float] = None
    t_to: Optional[float] = None
    deriv: bool = False


_VALUES = (Trace, Sample, Find)

_OF = {"minmax": abi.TIMING_MINMAX, "ends": abi.TIMING_ENDS}


@dataclass(frozen=True)
class Rel:
    frac: float
    of: int = abi.TIMING_MINMAX
    t_from: Optional[float] = None
    t_to: Optional[float] = None


@dataclass(frozen=True)
class Edge:
    signal: str
    level: object  # a float or a Rel
    dir: int = 1
    n: int = 1


@dataclass(frozen=True)
class When:
    edge: Edge
    t_from: Optional[float] = None
    t_to: Optional[float] = None

    def requests(self):
        return [(None, self.edge, False)]


@dataclass(frozen=True)
class Delay:
    trig: Edge
    targ: Edge
    after_trig: bool = True
    t_from: Optional[float] = None
    t_to: Optional[float] = None

    def requests(self):
        return [(self.trig, self.targ, self.after_trig)]


@dataclass(frozen=True)
class Transition:
    """rise_time / fall_time: from the first crossing of `start` to the first crossing of `end` at or after it."""
    start: Edge
    end: Edge
    t_from: Optional[float] = None
    t_to: Optional[float] = None

    def requests(self):
        return [(self.start, self.end, True)]


@dataclass(frozen=True)
class Settle:
    lo: Edge
    hi: Edge
    t_from: Optional[float] = None
    t_to: Optional[float] = None

    def requests(self):
        return [(None, self.lo, False), (None, self.hi, False)]


_TIMING = (When, Delay, Transition, Settle)


def rel(frac: float, of: str = "minmax", t_from: Optional[float] = None, t_to: Optional[float] = None) -> Rel:
    """A level relative to the signal's own swing in each circuit: lo + frac * (hi - lo), (lo, hi) = (min, max) for
    of="minmax", (first, last) for of="ends", over the base window [t_from, t_to] (default: the whole run)."""
    if of not in _OF:
        raise ValueError(f"rel: of must be 'minmax' or 'ends', got {of!r}")
    frac = float(frac)
    if not math.isfinite(frac):
        raise ValueError(f"rel: the fraction must be finite, got {frac!r}")
    return Rel(frac, _OF[of], t_from, t_to)


def edge(signal: str, level, dir="rise", n: int = 1) -> Edge:
    """The n-th crossing (n <= -1: the |n|-th from the end) of `level` (a number or rel(...)) by `signal`."""
    if dir not in _DIRS:
        raise ValueError(f"edge: dir must be 'rise', 'fall' or 'either', got {dir!r}")
    if isinstance(n, bool) or int(n) != n or int(n) == 0:
        raise ValueError(f"edge: n must be a nonzero integer, got {n!r}")
    if not isinstance(level, Rel):
        level = float(level)
        if not math.isfinite(level):
            raise ValueError(f"edge: the level must be finite, got {level!r}")
    return Edge(str(signal), level, _DIRS[dir], int(n))


def when(signal: str, level, dir="rise", n: int = 1, t_from: Optional[float] = None, t_to: Optional[float] = None) -> When:
    return When(edge(signal, level, dir, n), t_from, t_to)


def delay(trig: Edge, targ: Edge, after_trig: bool = True, t_from: Optional[float] = None, t_to: Optional[float] = None) -> Delay:
    if not isinstance(trig, Edge) or not isinstance(targ, Edge):
        raise TypeError("delay: trig and targ must be edge(...)")
    return Delay(trig, targ, bool(after_trig), t_from, t_to)


def rise_time(signal: str, lo: float = 0.1, hi: float = 0.9, of: str = "minmax", t_from: Optional[float] = None, t_to: Optional[float] = None) -> Transition:
    return Transition(edge(signal, rel(lo, of), "rise"), edge(signal, rel(hi, of), "rise"), t_from, t_to)


def fall_time(signal: str, lo: float = 0.1, hi: float = 0.9, of: str = "minmax", t_from: Optional[float] = None, t_to: Optional[float] = None) -> Transition:
    return Transition(edge(signal, rel(hi, of), "fall"), edge(signal, rel(lo, of), "fall"), t_from, t_to)


def settle(signal: str, tol: float = 0.02, t_from: Optional[float] = None, t_to: Optional[float] = None) -> Settle:
    tol = float(tol)
    if not (math.isfinite(tol) and tol > 0):
        raise ValueError(f"settle: tol must be finite and > 0, got {tol!r}")
    return Settle(edge(signal, rel(1.0 - tol, "ends"), "either", -1), edge(signal, rel(1.0 + tol, "ends"), "either", -1), t_from, t_to)


_NO_EDGE = (0, 0, -1, 1, 1, 0, 0, 0, 0.0)


def make_timing_reqs(rows: Sequence[tuple]) -> np.ndarray:
    """Request records (abi.TIMING_REQ_DTYPE) from tuples (step_from, step_to, trig, targ, targ_from_trig) with trig (None:
    has_trig = 0) and targ tuples (signal, col, col_ref, dir, n, level_kind, base_from, base_to, level)."""
    a = np.zeros(len(rows), abi.TIMING_REQ_DTYPE)
    for k, (s0, s1, trig, targ, from_trig) in enumerate(rows):
        a[k] = (s0, s1, 0 if trig is None else 1, int(from_trig), tuple(_NO_EDGE if trig is None else trig), tuple(targ))
    return a


def stats(signal: str, t_from: Optional[float] = None, t_to: Optional[float] = None) -> Stats:
    return Stats(str(signal), t_from, t_to)


def cross(signal: str, level: float, dir="rise", t_from: Optional[float] = None, t_to: Optional[float] = None) -> Cross:
    if dir not in _DIRS:
        raise ValueError(f"cross: dir must be 'rise', 'fall' or 'either', got {dir!r}")
    return Cross(str(signal), float(level), _DIRS[dir], t_from, t_to)


def fourier(signal: str, f0: float, harmonics: int = 9, t_from: Optional[float] = None, t_to: Optional[float] = None,
            periods: Optional[int] = None) -> Fourier:
    f0 = float(f0)
    if not (math.isfinite(f0) and f0 > 0):
        raise ValueError(f"fourier: f0 must be finite and > 0, got {f0!r}")
    if isinstance(harmonics, bool) or int(harmonics) != harmonics or not 1 <= int(harmonics) <= abi.FOUR_MAX_HARM:
        raise ValueError(f"fourier: harmonics must be an integer in 1..{abi.FOUR_MAX_HARM}, got {harmonics!r}")
    if periods is not None:
        if t_from is not None:
            raise ValueError("fourier: give periods= or t_from=, not both (periods counts back from t_to)")
        if isinstance(periods, bool) or int(periods) != periods or int(periods) < 1:
            raise ValueError(f"fourier: periods must be an integer >= 1, got {periods!r}")
        periods = int(periods)
    return Fourier(str(signal), f0, int(harmonics), t_from, t_to, periods)


def _spectrum_spec(who: str, kind: int, signal, n, window, f_from, f_to, t_from, t_to) -> Spectrum:
    if window not in _WINDOWS:
        raise ValueError(f"{who}: window must be 'hann' or 'rect', got {window!r}")
    if n is not None:
        if isinstance(n, bool) or int(n) != n or not (1 << abi.SPEC_MIN_LOG2N) <= int(n) <= (1 << abi.SPEC_MAX_LOG2N) or int(n) & (int(n) - 1):
            raise ValueError(f"{who}: n must be a power of two in {1 << abi.SPEC_MIN_LOG2N}..{1 << abi.SPEC_MAX_LOG2N}, got {n!r}")
        n = int(n)
    for nm, f in (("f_from", f_from), ("f_to", f_to)):
        if f is not None and not (math.isfinite(float(f)) and float(f) >= 0):
            raise ValueError(f"{who}: {nm} must be finite and >= 0, got {f!r}")
    return Spectrum(str(signal), n, _WINDOWS[window], None if f_from is None else float(f_from), None if f_to is None else float(f_to), t_from, t_to, kind)


def spectrum(signal: str, n: Optional[int] = None, window: str = "hann", f_from: Optional[float] = None, f_to: Optional[float] = None,
             t_from: Optional[float] = None, t_to: Optional[float] = None) -> Spectrum:
    """The band's bins of the n-point FFT of the window's last n samples: {n, df, window, freq[], mag[], phase_deg[]}.  The
    phases refer to the window's FIRST sample (fourier()'s refer to t = 0); see the module text."""
    return _spectrum_spec("spectrum", abi.SPEC_BINS, signal, n, window, f_from, f_to, t_from, t_to)


def dominant(signal: str, n: Optional[int] = None, window: str = "hann", f_from: Optional[float] = None, f_to: Optional[float] = None,
             t_from: Optional[float] = None, t_to: Optional[float] = None) -> Spectrum:
    """The band's strongest bin, found on the device: {bin, freq, mag, freq_bin, n, df}; DC is excluded unless f_from says
    otherwise; see the module text."""
    return _spectrum_spec("dominant", abi.SPEC_DOMINANT, signal, n, window, f_from, f_to, t_from, t_to)


def power(a: str, b: Optional[str] = None, *, t_from: Optional[float] = None, t_to: Optional[float] = None) -> Power:
    """power("R1"): the power the element absorbs, v(n1,n2) i(R1) (passive sign convention); power("v(out)", "i(Rload)"): the
    product of any two signals.  {energy, avg, peak, t_peak, min, t_min, first, final, rms_a, rms_b, apparent, pf}; see the
    module text."""
    if not isinstance(a, str) or (b is not None and not isinstance(b, str)):
        raise TypeError("power: an element name, or two signals")
    return Power(a, b, t_from, t_to)


def efficiency(load, source, *, t_from: Optional[float] = None, t_to: Optional[float] = None) -> Efficiency:
    """avg power into `load` over avg power out of `source`, each an element name or a power(...) spec: {p_load, p_source,
    eff}; see the module text."""
    parts = []
    for p in (load, source):
        if not isinstance(p, (str, Power)):
            raise TypeError(f"efficiency: load and source must be element names or power(...), got {type(p).__name__}")
        parts.append(power(p) if isinstance(p, str) else p)
    return Efficiency(parts[0], parts[1], t_from, t_to)


def trace(signal: str, buckets: int = 512, t_from: Optional[float] = None, t_to: Optional[float] = None) -> Trace:
    """The window's waveform decimated to min / max / first / last per bucket, and the polyline t[] / v[] to plot; see the
    module text."""
    if isinstance(buckets, bool) or int(buckets) != buckets or int(buckets) < 1:
        raise ValueError(f"trace: buckets must be an integer >= 1, got {buckets!r}")
    return Trace(str(signal), int(buckets), t_from, t_to)


def sample(signal: str, times) -> Sample:
    """The signal interpolated linearly at the given times: {t[], value[], slope[]}; see the module text."""
    ts = tuple(float(t) for t in np.asarray(times, dtype=np.float64).reshape(-1))
    if not ts:
        raise ValueError("sample: no times given")
    if not all(math.isfinite(t) for t in ts):
        raise ValueError("sample: the times must be finite")
    return Sample(str(signal), ts)


def _find_spec(who: str, signal, when, at, t_from, t_to, is_deriv: bool) -> Find:
    if (when is None) == (at is None):
        raise ValueError(f"{who}: give when=edge(...) or at=t, one of them")
    if when is not None:
        if not isinstance(when, Edge):
            raise TypeError(f"{who}: when must be edge(...)")
        return Find(str(signal), when, None, t_from, t_to, is_deriv)
    if t_from is not None or t_to is not None:
        raise ValueError(f"{who}: t_from / t_to go with when=, not with at=")
    at = float(at)
    if not math.isfinite(at):
        raise ValueError(f"{who}: at must be finite, got {at!r}")
    return Find(str(signal), None, at, None, None, is_deriv)


def find(signal: str, when: Optional[Edge] = None, at: Optional[float] = None, t_from: Optional[float] = None, t_to: Optional[float] = None) -> Find:
    """The signal's value and slope where another signal crosses a level (when=edge(...)) or at a time (at=t): {t, value,
    slope, level, count}; see the module text."""
    return _find_spec("find", signal, when, at, t_from, t_to, False)


def deriv(signal: str, when: Optional[Edge] = None, at: Optional[float] = None, t_from: Optional[float] = None, t_to: Optional[float] = None) -> Find:
    """find(...) with the slope returned as `value`."""
    return _find_spec("deriv", signal, when, at, t_from, t_to, True)


def make_value_reqs(rows: Sequence[tuple]) -> np.ndarray:
    """Request records (abi.VAL_REQ_DTYPE) from tuples (kind, signal, col, col_ref, x_signal, x_col, x_col_ref, timing_row,
    step_from, step_to, first, count, buckets)."""
    a = np.zeros(len(rows), abi.VAL_REQ_DTYPE)
    for k, r in enumerate(rows):
        a[k] = tuple(r) + (0,)
    return a


def make_value_points(points: Sequence[tuple]) -> np.ndarray:
    """Point records (abi.VAL_POINT_DTYPE) from tuples (k, f)."""
    a = np.zeros(len(points), abi.VAL_POINT_DTYPE)
    for j, kf in enumerate(points):
        a[j] = tuple(kf)
    return a


def time_to_point(t: float, dt: float, steps: int, name: str = "") -> Tuple[int, float, float]:
    """(k, f, the time it stands for) of a sample time in a run of `steps` steps of dt (module text), or ValueError."""
    if steps < 1:
        raise ValueError(f"measure {name!r}: a run of one point has no interval to interpolate in")
    q = t / dt
    if not (-0.5 < q < steps + 0.5):
        raise ValueError(f"measure {name!r}: the time {t!r} lies half a step or more outside the run [0, {steps * dt!r}]")
    if q < 0.0:
        q, t = 0.0, 0.0
    elif q > steps:
        q, t = float(steps), steps * dt
    k = min(int(math.floor(q)), steps - 1)
    return k, q - k, float(t)


def make_power_reqs(rows: Sequence[tuple]) -> np.ndarray:
    """Request records (abi.POWER_REQ_DTYPE) from tuples (a_signal, a_col, a_col_ref, b_signal, b_col, b_col_ref, neg, step_from,
    step_to)."""
    a = np.zeros(len(rows), abi.POWER_REQ_DTYPE)
    for k, r in enumerate(rows):
        a[k] = tuple(r[:7]) + (0,) + tuple(r[7:])
    return a


def make_spec_reqs(rows: Sequence[tuple]) -> np.ndarray:
    """Request records (abi.SPEC_REQ_DTYPE) from tuples (signal, col, col_ref, kind, step_from, log2n, window, bin_from, bin_to)."""
    a = np.zeros(len(rows), abi.SPEC_REQ_DTYPE)
    for k, r in enumerate(rows):
        a[k] = tuple(r)
    return a


def spectrum_window(spec: Spectrum, dt: float, steps: int, name: str = "") -> Tuple[int, int, int, int]:
    """(step_from, log2n, bin_from, bin_to) of a spectrum / dominant spec in a run of `steps` steps of dt, or ValueError
    (module text)."""
    s0 = time_to_step(spec.t_from, dt, steps, 0)
    s1 = time_to_step(spec.t_to, dt, steps, steps)
    count = s1 - s0 + 1
    n = spec.n
    if n is None:
        if count < (1 << abi.SPEC_MIN_LOG2N):
            raise ValueError(f"measure {name!r}: the window of {max(count, 0)} samples is shorter than the shortest transform of {1 << abi.SPEC_MIN_LOG2N}")
        n = min(1 << (count.bit_length() - 1), 1 << abi.SPEC_MAX_LOG2N)
    elif n > count:
        raise ValueError(f"measure {name!r}: n = {n} is longer than the window of {max(count, 0)} samples")
    half = n // 2
    # (dominant()'s default lower edge is df = bin 1, set as a bin: df N dt need not round to 1.0)
    b0 = (1 if spec.kind == abi.SPEC_DOMINANT else 0) if spec.f_from is None else math.ceil(spec.f_from * n * dt)
    b1 = half if spec.f_to is None else math.floor(spec.f_to * n * dt)
    # (a lower edge above Nyquist leaves no bin: the clamp is for an upper edge beyond it)
    if b0 > half or b0 > b1:
        raise ValueError(f"measure {name!r}: no bin of the {n}-point transform (df = {1.0 / (n * dt)} Hz) lies in the band [{spec.f_from}, {spec.f_to}] Hz")
    return s1 - n + 1, n.bit_length() - 1, max(b0, 0), min(b1, half)


def make_four_reqs(rows: Sequence[tuple]) -> np.ndarray:
    """Request records (abi.FOUR_REQ_DTYPE) from tuples (signal, col, col_ref, n_harm, step_from, step_to, f0)."""
    a = np.zeros(len(rows), abi.FOUR_REQ_DTYPE)
    for k, r in enumerate(rows):
        a[k] = tuple(r)
    return a


def fourier_window(spec: Fourier, dt: float, steps: int, name: str = "") -> Tuple[int, int]:
    """(step_from, step_to) of a fourier spec in a run of `steps` steps of dt, or ValueError (module text)."""
    if spec.harmonics * spec.f0 > 1.0 / (2.0 * dt):
        raise ValueError(f"measure {name!r}: harmonic {spec.harmonics} of {spec.f0} Hz is above Nyquist, 1 / (2 dt) = {1.0 / (2.0 * dt)} Hz")
    s1 = time_to_step(spec.t_to, dt, steps, steps)
    s0 = s1 - int(round(spec.periods / (spec.f0 * dt))) if spec.periods is not None else time_to_step(spec.t_from, dt, steps, 0)
    if s0 < 0:
        raise ValueError(f"measure {name!r}: {spec.periods} periods of {spec.f0} Hz before step {s1} reach before the run")
    if s0 >= s1:
        raise ValueError(f"measure {name!r}: the window is empty (it starts at step {s0} and ends at step {s1})")
    if (s1 - s0 + 0.5) * dt * spec.f0 < 1.0:
        raise ValueError(f"measure {name!r}: the window of {s1 - s0} steps is shorter than one period of {spec.f0} Hz")
    return s0, s1


def make_reqs(rows: Sequence[tuple]) -> np.ndarray:
    """Request records (abi.MEAS_REQ_DTYPE) from tuples (kind, signal, col, col_ref, step_from, step_to, level, dir)."""
    a = np.zeros(len(rows), abi.MEAS_REQ_DTYPE)
    for k, r in enumerate(rows):
        a[k] = tuple(r) + (0,)
    return a


def time_to_step(t: Optional[float], dt: float, steps: int, default: int) -> int:
    """The window rule of the module text: nearest step, ties to the later one, clamped to the run."""
    if t is None:
        return default
    return int(min(max(math.floor(t / dt + 0.5), 0), steps))


_SIGNAL = re.compile(r"^\s*([vi])\s*\(\s*([^,()\s]+)\s*(?:,\s*([^,()\s]+)\s*)?\)\s*$", re.I)


def _element_names(ckt: ParsedCircuit) -> List[str]:
    # simulateTRAN's recording order (R, C, L, V, S, D): the columns of out_i
    return ([e.name for e in ckt.R] + [e.name for e in ckt.C] + [e.name for e in ckt.L] + [e.name for e in ckt.V]
            + [e.name for e in ckt.S if e.model is not None] + [e.name for e in ckt.D if e.model is not None])


def _parse_signal(ckt: ParsedCircuit, text: str, elements: Optional[List[str]] = None) -> Tuple[int, int, int]:
    """(signal, a, b): signal 0 -> node ids a and b (b = 0: none); signal 1 -> out_i column a.  elements: the names of the
    out_i columns (default: the transient's recording order)."""
    m = _SIGNAL.match(text)
    if not m:
        raise ValueError(f"measure: cannot read the signal {text!r} (v(node), v(node,node) or i(element))")
    kind, a, b = m.group(1).lower(), m.group(2), m.group(3)
    if kind == "i":
        if b is not None:
            raise ValueError(f"measure: {text!r}: i() takes one element name")
        hits = [k for k, nm in enumerate(_element_names(ckt) if elements is None else elements) if nm.upper() == a.upper()]
        if not hits:
            raise ValueError(f"measure: {text!r}: no element named {a!r} records a current")
        if len(hits) > 1:
            raise ValueError(f"measure: {text!r}: {len(hits)} elements share the name {a!r}")
        return 1, hits[0], 0
    ids = []
    for nm in (a, b):
        if nm is None:
            ids.append(0)
            continue
        i = ckt.nodes.get(nm)
        if i is None:
            raise ValueError(f"measure: {text!r}: no node named {nm!r}")
        ids.append(i)
    if ids[0] == 0:
        raise ValueError(f"measure: {text!r}: the first node is ground")
    return 0, ids[0], ids[1]


def _element_terminals(ckt: ParsedCircuit) -> List[Tuple[str, int, int]]:
    # (name, first terminal, second terminal) of the out_i columns, in _element_names' order; the recorded current flows
    # from the first to the second
    return ([(e.name, e.n1, e.n2) for e in ckt.R] + [(e.name, e.n1, e.n2) for e in ckt.C] + [(e.name, e.n1, e.n2) for e in ckt.L]
            + [(e.name, e.n1, e.n2) for e in ckt.V] + [(e.name, e.n1, e.n2) for e in ckt.S if e.model is not None]
            + [(e.name, e.nPlus, e.nMinus) for e in ckt.D if e.model is not None])


def _power_factors(ckt: ParsedCircuit, spec: Power) -> Tuple[Tuple[int, int, int], Tuple[int, int, int], int]:
    """(factor a, factor b, neg) of a power spec, the factors as _parse_signal's (signal, a, b)."""
    if spec.b is not None:
        return _parse_signal(ckt, spec.a), _parse_signal(ckt, spec.b), 0
    name = spec.a.strip()
    hits = [(k, n1, n2) for k, (nm, n1, n2) in enumerate(_element_terminals(ckt)) if nm.upper() == name.upper()]
    if not hits:
        raise ValueError(f"measure: power({spec.a!r}): no element named {name!r} records a current")
    if len(hits) > 1:
        raise ValueError(f"measure: power({spec.a!r}): {len(hits)} elements share the name {name!r}")
    k, n1, n2 = hits[0]
    if n1 == 0 and n2 == 0:
        raise ValueError(f"measure: power({spec.a!r}): both terminals of {name!r} are ground")
    # (v(0,n2) i = -(v(n2) i): the first node of a recorded difference is never ground)
    return ((0, n1, n2), (1, k, 0), 0) if n1 != 0 else ((0, n2, 0), (1, k, 0), 1)


class _Plan:
    """A circuit's measures resolved: the recorded nodes, whether currents are needed, the request records."""

    def __init__(self, ckt: ParsedCircuit, measures: Dict[str, object], dt: float, steps: int):
        if not measures:
            raise ValueError("measure: no measures given")
        parsed = []
        negs = {}  # name -> neg of each product request of a power / efficiency spec
        for name, spec in measures.items():
            if isinstance(spec, _PRODUCTS):
                # (the two factors of every product request, resolved: a list in the place of the one signal)
                factors = [_power_factors(ckt, p) for p in spec.parts()]
                parsed.append((name, spec, [f[:2] for f in factors]))
                negs[name] = [f[2] for f in factors]
                continue
            if isinstance(spec, _TIMING):
                # (every edge of the spec's requests, resolved: a list in the place of the one signal)
                parsed.append((name, spec, [tuple(None if e is None else _parse_signal(ckt, e.signal) for e in rq[:2]) for rq in spec.requests()]))
                continue
            if isinstance(spec, _VALUES):
                # (the signal and, for find(when=), the edge's own: a list as above)
                x = _parse_signal(ckt, spec.when.signal) if isinstance(spec, Find) and spec.when is not None else None
                parsed.append((name, spec, [(_parse_signal(ckt, spec.signal), x)]))
                continue
            if not isinstance(spec, (Stats, Cross, Fourier, Spectrum)):
                raise TypeError(f"measure {name!r}: expected stats(...), cross(...), fourier(...), when(...), delay(...), rise_time(...), "
                                f"fall_time(...), settle(...), spectrum(...), dominant(...), power(...), efficiency(...), trace(...), sample(...), find(...) or "
                                f"deriv(...), got {type(spec).__name__}")
            parsed.append((name, spec, _parse_signal(ckt, spec.signal)))
        sigs = [s for _, _, p in parsed for s in ([e for rq in p for e in rq if e is not None] if isinstance(p, list) else [p])]
        nodes = sorted({n for sig, a, b in sigs if sig == 0 for n in (a, b) if n != 0})
        self.need_i = any(sig == 1 for sig, _, _ in sigs)
        # (a device descriptor records at least one node; with current measures only, the first one)
        self.out_nodes = nodes if nodes else [1]
        col = {n: c for c, n in enumerate(self.out_nodes)}
        rows, frows, trows, srows, prows, vrows, vpts = [], [], [], [], [], [], []
        # (name, "meas" | "four" | "spec" | the timing or product spec, its (first) place in reqs / freqs / sreqs / treqs / preqs), in the dict's order
        self.names = []

        def columns(sig, a, b):
            return (col[a], col[b] if b else -1) if sig == 0 else (a, -1)

        def edge_row(name, e: Edge, where):
            sig = where[0]
            c, cr = columns(*where)
            if isinstance(e.level, Rel):
                b0 = time_to_step(e.level.t_from, dt, steps, 0)
                b1 = time_to_step(e.level.t_to, dt, steps, steps)
                if b0 > b1:
                    raise ValueError(f"measure {name!r}: the base window of rel() is empty (t_from maps to step {b0}, t_to to step {b1})")
                return (sig, c, cr, e.dir, e.n, e.level.of, b0, b1, e.level.frac)
            return (sig, c, cr, e.dir, e.n, abi.TIMING_ABS, 0, 0, e.level)

        for name, spec, where in parsed:
            if isinstance(spec, _VALUES):
                ysig, xsig = where[0]
                head = (ysig[0],) + columns(*ysig)
                self.names.append((name, spec, len(vrows)))
                if isinstance(spec, Trace):
                    s0 = time_to_step(spec.t_from, dt, steps, 0)
                    s1 = time_to_step(spec.t_to, dt, steps, steps)
                    if s0 > s1:
                        raise ValueError(f"measure {name!r}: the window is empty (t_from maps to step {s0}, t_to to step {s1})")
                    B = min(spec.buckets, s1 - s0 + 1)
                    if B > abi.TRACE_MAX_BUCKETS:
                        raise ValueError(f"measure {name!r}: {B} buckets are more than abi.TRACE_MAX_BUCKETS = {abi.TRACE_MAX_BUCKETS}")
                    vrows.append((abi.VAL_TRACE,) + head + (0, 0, -1, 0, s0, s1, 0, 0, B))
                elif isinstance(spec, Sample) or spec.when is None:
                    ts = spec.times if isinstance(spec, Sample) else (spec.at,)
                    vrows.append((abi.VAL_POINTS,) + head + (0, 0, -1, 0, 0, 0, len(vpts), len(ts), 0))
                    vpts += [time_to_point(t, dt, steps, name) for t in ts]
                else:
                    s0 = time_to_step(spec.t_from, dt, steps, 0)
                    s1 = time_to_step(spec.t_to, dt, steps, steps)
                    if s0 >= s1:
                        raise ValueError(f"measure {name!r}: the window has no interval (t_from maps to step {s0}, t_to to step {s1})")
                    # (one hidden targ-only request of the timing list, as rise_time composes its own)
                    vrows.append((abi.VAL_FIND,) + head + (xsig[0],) + columns(*xsig) + (len(trows), 0, 0, 0, 0, 0))
                    trows.append((s0, s1, None, edge_row(name, spec.when, xsig), False))
                continue
            if isinstance(spec, _PRODUCTS):
                self.names.append((name, spec, len(prows)))
                for part, (fa, fb), neg in zip(spec.parts(), where, negs[name]):
                    s0 = time_to_step(part.t_from, dt, steps, 0)
                    s1 = time_to_step(part.t_to, dt, steps, steps)
                    if s0 > s1:
                        raise ValueError(f"measure {name!r}: the window is empty (t_from maps to step {s0}, t_to to step {s1})")
                    prows.append((fa[0],) + columns(*fa) + (fb[0],) + columns(*fb) + (neg, s0, s1))
                continue
            if isinstance(spec, _TIMING):
                s0 = time_to_step(spec.t_from, dt, steps, 0)
                s1 = time_to_step(spec.t_to, dt, steps, steps)
                if s0 >= s1:
                    raise ValueError(f"measure {name!r}: the window has no interval (t_from maps to step {s0}, t_to to step {s1})")
                self.names.append((name, spec, len(trows)))
                for (trig, targ, from_trig), (w_trig, w_targ) in zip(spec.requests(), where):
                    trows.append((s0, s1, None if trig is None else edge_row(name, trig, w_trig), edge_row(name, targ, w_targ), from_trig))
                continue
            sig, a, b = where
            c, cr = columns(sig, a, b)
            if isinstance(spec, Fourier):
                s0, s1 = fourier_window(spec, dt, steps, name)
                self.names.append((name, "four", len(frows)))
                frows.append((sig, c, cr, spec.harmonics, s0, s1, spec.f0))
                continue
            if isinstance(spec, Spectrum):
                s0, log2n, b0, b1 = spectrum_window(spec, dt, steps, name)
                self.names.append((name, "spec", len(srows)))
                srows.append((sig, c, cr, spec.kind, s0, log2n, spec.window, b0, b1))
                continue
            s0 = time_to_step(spec.t_from, dt, steps, 0)
            s1 = time_to_step(spec.t_to, dt, steps, steps)
            if s0 > s1:
                raise ValueError(f"measure {name!r}: the window is empty (t_from maps to step {s0}, t_to to step {s1})")
            self.names.append((name, "meas", len(rows)))
            if isinstance(spec, Stats):
                rows.append((abi.MEAS_STATS, sig, c, cr, s0, s1, 0.0, 0))
            else:
                rows.append((abi.MEAS_CROSS, sig, c, cr, s0, s1, spec.level, spec.dir))
        self.reqs = make_reqs(rows)
        self.freqs = make_four_reqs(frows)  # (empty: the dict takes the path without the harmonics pass)
        self.treqs = make_timing_reqs(trows)  # (empty: the dict takes the path without the timing pass)
        self.sreqs = make_spec_reqs(srows)  # (empty: the dict takes the path without the spectrum pass)
        self.preqs = make_power_reqs(prows)  # (empty: the dict takes the path without the product pass)
        self.vreqs = make_value_reqs(vrows)  # (empty: the dict takes the path without the values pass)
        self.pts = make_value_points([p[:2] for p in vpts])
        self.pt_times = [p[2] for p in vpts]  # the time each point of the table stands for

    def flatten(self, ckt: ParsedCircuit) -> abi.FlatCircuit:
        flat = abi.flatten(ckt)
        flat.out_nodes = np.ascontiguousarray(self.out_nodes, dtype=np.int32)
        return flat

    def key(self) -> bytes:
        """What a batch groups by beside topology and run: the resolved request tables."""
        key = self.reqs.tobytes() + b"|" + self.freqs.tobytes() + (b"|" + self.treqs.tobytes() if len(self.treqs) else b"")
        key = key + b"|s|" + self.sreqs.tobytes() if len(self.sreqs) else key
        key = key + b"|p|" + self.preqs.tobytes() if len(self.preqs) else key
        return key + b"|v|" + self.vreqs.tobytes() + b"|" + self.pts.tobytes() if len(self.vreqs) else key

    def run(self, be, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray) -> dict:
        if len(self.vreqs):
            return backend_reduce(be, flat, steps, dt, src, self.reqs, self.freqs, self.treqs, self.need_i, self.sreqs, self.preqs, self.vreqs, self.pts)
        return backend_reduce(be, flat, steps, dt, src, self.reqs, self.freqs, self.treqs, self.need_i, self.sreqs, self.preqs)

    def values(self, res: dict, j: int, dt: float) -> Dict[str, dict]:
        """Instance j of a result (meas [n_inst][n_req][8], four [n_inst][n_four][row], timing [n_inst][n_timing][8], spec
        [n_inst][n_spec][row], power [n_inst][n_power][16]) -> {name: {...}}."""
        return {name: derive(self.reqs[k], res["meas"][j][k], dt) if kind == "meas" else derive_fourier(self.freqs[k], res["four"][j][k], dt)
                if kind == "four" else derive_spectrum(self.sreqs[k], res["spec"][j][k], dt) if kind == "spec"
                else derive_power(self.preqs[k], res["power"][j][k], dt) if isinstance(kind, Power)
                else derive_efficiency(self.preqs[k:k + 2], res["power"][j][k:k + 2], dt) if isinstance(kind, Efficiency)
                else derive_values(kind, self.vreqs[k], res["values"][j][k], dt, self.pt_times, res["timing"][j]) if isinstance(kind, _VALUES)
                else derive_timing(kind, res["timing"][j][k:k + len(kind.requests())])
                for name, kind, k in self.names}


def derive(req, m, dt: float) -> dict:
    """The values of one measure from its 8 doubles (module text)."""
    if int(req["kind"]) == abi.MEAS_STATS:
        mn, mx, smn, smx, s, sq, first, last = (float(v) for v in m)
        n = int(req["step_to"]) - int(req["step_from"]) + 1
        if n > 1:
            span = (n - 1) * dt
            integ = dt * (s - (first + last) / 2)
            avg = integ / span
            rms = math.sqrt(max(dt * (sq - (first * first + last * last) / 2) / span, 0.0))
        else:
            integ, avg, rms = 0.0, first, abs(first)
        return {"min": mn, "max": mx, "pp": mx - mn, "t_min": smn * dt, "t_max": smx * dt, "first": first, "final": last,
                "integ": integ, "avg": avg, "rms": rms}
    count = int(m[0])
    tf, tl = (float(m[1]), float(m[2])) if count > 0 else (None, None)
    freq = (count - 1) / (tl - tf) if count >= 2 and tl > tf else None
    return {"count": count, "t_first": tf, "t_last": tl, "freq": freq}


def trace_buckets(req, n_points: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(first step, last step) of every bucket of a trace request, as int64 arrays; n_points resolves step_to = -1."""
    s0, s1, B = int(req["step_from"]), int(req["step_to"]), int(req["buckets"])
    if s1 == -1:
        s1 = n_points - 1
    n = s1 - s0 + 1
    edges = s0 + np.arange(B + 1, dtype=np.int64) * n // B
    return edges[:-1], edges[1:] - 1


def derive_values(spec, req, row, dt: float, pt_times: Sequence[float], timing) -> dict:
    """The values of one trace / sample / find spec from its row (module text); pt_times: the time of every point of the
    plan's table; timing: the instance's timing rows (find(when=) reads its hidden request's)."""
    if isinstance(spec, Trace):
        B = int(req["buckets"])
        lo, hi = trace_buckets(req)
        r = np.asarray(row[:abi.VAL_TRACE_DOUBLES * B], dtype=np.float64).reshape(B, abi.VAL_TRACE_DOUBLES)
        # per bucket first, min, max, last in step order (a stable sort: of equal steps the earlier of that list stays)
        st = np.stack([lo.astype(np.float64), r[:, 1], r[:, 3], hi.astype(np.float64)], axis=1)
        vs = np.stack([r[:, 4], r[:, 0], r[:, 2], r[:, 5]], axis=1)
        order = np.argsort(st, axis=1, kind="stable")
        st, vs = np.take_along_axis(st, order, axis=1), np.take_along_axis(vs, order, axis=1)
        keep = np.ones_like(st, dtype=bool)
        keep[:, 1:] = st[:, 1:] != st[:, :-1]
        return {"buckets": B, "t_first": (lo * dt).tolist(), "first": r[:, 4].tolist(), "t_min": (r[:, 1] * dt).tolist(), "min": r[:, 0].tolist(),
                "t_max": (r[:, 3] * dt).tolist(), "max": r[:, 2].tolist(), "t_last": (hi * dt).tolist(), "last": r[:, 5].tolist(),
                "t": (st[keep] * dt).tolist(), "v": vs[keep].tolist()}
    if isinstance(spec, Sample):
        first, count = int(req["first"]), int(req["count"])
        r = np.asarray(row[:abi.VAL_POINT_DOUBLES * count], dtype=np.float64).reshape(count, abi.VAL_POINT_DOUBLES)
        return {"t": list(pt_times[first:first + count]), "value": r[:, 2].tolist(), "slope": r[:, 3].tolist()}
    k, f, value, slope = (float(v) for v in row[:4])
    if spec.when is None:
        t, level, count = pt_times[int(req["first"])], None, None
    else:
        trow = timing[int(req["timing_row"])]
        t, level, count = ((k + f) * dt if k >= 0 else None), float(trow[5]), int(trow[7])
        if k < 0:
            value = slope = None
    return {"t": t, "value": slope if spec.deriv else value, "slope": slope, "level": level, "count": count}


def derive_power(req, row, dt: float) -> dict:
    """The values of one power spec from its 16 doubles (module text)."""
    mn, mx, smn, smx, s, first, last, saa, sbb, fa, la, fb, lb = (float(v) for v in row[:13])
    n = int(req["step_to"]) - int(req["step_from"]) + 1
    if n > 1:
        span = (n - 1) * dt
        energy = dt * (s - (first + last) / 2)
        avg = energy / span
        rms_a = math.sqrt(max(dt * (saa - (fa * fa + la * la) / 2) / span, 0.0))
        rms_b = math.sqrt(max(dt * (sbb - (fb * fb + lb * lb) / 2) / span, 0.0))
    else:
        energy, avg, rms_a, rms_b = 0.0, first, abs(fa), abs(fb)
    apparent = rms_a * rms_b
    return {"energy": energy, "avg": avg, "peak": mx, "t_peak": smx * dt, "min": mn, "t_min": smn * dt, "first": first, "final": last,
            "rms_a": rms_a, "rms_b": rms_b, "apparent": apparent, "pf": avg / apparent if apparent != 0.0 else None}


def derive_efficiency(reqs, rows, dt: float) -> dict:
    """The values of one efficiency spec from the rows of its two product requests, load then source (module text)."""
    p_load = derive_power(reqs[0], rows[0], dt)["avg"]
    p_source = -derive_power(reqs[1], rows[1], dt)["avg"]
    return {"p_load": p_load, "p_source": p_source, "eff": p_load / p_source if p_source != 0.0 else None}


def derive_fourier(req, row, dt: float) -> dict:
    """The values of one fourier spec from its row {C0, C1, S1, ...} (module text)."""
    n = int(req["step_to"]) - int(req["step_from"])
    H, f0 = int(req["n_harm"]), float(req["f0"])
    mag, ph = [], []
    for h in range(1, H + 1):
        a, b = 2.0 * float(row[2 * h - 1]) / n, 2.0 * float(row[2 * h]) / n
        mag.append(math.hypot(a, b))
        ph.append(math.degrees(math.atan2(-b, a)))
    thd = math.sqrt(sum(m * m for m in mag[1:])) / mag[0] if H > 1 and mag[0] != 0.0 else None
    return {"f0": f0, "periods": n * dt * f0, "dc": float(row[0]) / n, "mag": mag, "phase_deg": ph, "thd": thd}


@functools.lru_cache(maxsize=None)
def spectrum_tables(log2n: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(T_re[N/2], T_im[N/2], w[N]) of include/spicey_hip.h for N = 2^log2n, by this process's libm (math.cos / math.sin: the
    functions the library's host code calls): T[k] = (cos(a_k), -sin(a_k)), w_j = 0.5 - 0.5 cos(a_j), a_k = (2.0 pi k) / N,
    T[0] and T[N/4] exact.  Read-only arrays."""
    N = 1 << log2n
    ang = [((2.0 * math.pi) * float(k)) / float(N) for k in range(N)]
    t_re = np.array([math.cos(a) for a in ang[:N // 2]])
    t_im = np.array([-math.sin(a) for a in ang[:N // 2]])
    t_re[0], t_im[0], t_re[N // 4], t_im[N // 4] = 1.0, 0.0, 0.0, -1.0
    w = np.array([0.5 - 0.5 * math.cos(a) for a in ang])
    for a in (t_re, t_im, w):
        a.setflags(write=False)
    return t_re, t_im, w


def _spectrum_scale(req) -> Tuple[int, float]:
    """(N, sum of the window's N weights) of a request."""
    N = 1 << int(req["log2n"])
    sw = math.fsum(spectrum_tables(int(req["log2n"]))[2].tolist()) if int(req["window"]) == abi.SPEC_HANN else float(N)
    return N, sw


def derive_spectrum(req, row, dt: float) -> dict:
    """The values of one spectrum / dominant spec from its row (module text)."""
    N, sw = _spectrum_scale(req)
    df = 1.0 / (N * dt)

    def side(k):
        return 1.0 if k == 0 or k == N // 2 else 2.0

    if int(req["kind"]) == abi.SPEC_BINS:
        b0, b1 = int(req["bin_from"]), int(req["bin_to"])
        ks = list(range(b0, b1 + 1))
        re_, im_ = [float(v) for v in row[0:2 * len(ks):2]], [float(v) for v in row[1:2 * len(ks):2]]
        return {"n": N, "df": df, "window": _WINDOW_NAMES[int(req["window"])], "freq": [k * df for k in ks],
                "mag": [math.hypot(a, b) * side(k) / sw for k, a, b in zip(ks, re_, im_)],
                "phase_deg": [math.degrees(math.atan2(b, a)) for a, b in zip(re_, im_)]}
    k = int(row[0])
    if k < 0:
        return {"bin": None, "freq": None, "mag": None, "freq_bin": None, "n": None, "df": None}
    pa, pb, pc = float(row[3]), float(row[4]), float(row[5])
    d = 0.0
    if pa >= 0.0 and pc >= 0.0:
        a, b, c = math.sqrt(pa), math.sqrt(pb), math.sqrt(pc)
        den = a - 2.0 * b + c
        if den != 0.0:
            d = 0.5 * (a - c) / den
    return {"bin": k, "freq": (k + d) * df, "mag": math.sqrt(pb) * side(k) / sw, "freq_bin": k * df, "n": N, "df": df}


def reduce_reference_spectrum(out_v: np.ndarray, out_i: Optional[np.ndarray], reqs, dt: float) -> np.ndarray:
    """The definition of spicey_spectrum_device in vectorised numpy: out_v [n_inst][n_points][n_v], out_i likewise or None,
    reqs records of abi.SPEC_REQ_DTYPE -> [n_inst][n_req][row], row = the longest request's, zeros behind a request's own.
    The same elementwise IEEE operations on the same operands as the device's (every product, sum and difference a numpy
    operation of its own), whole stages at a time, the tables by this process's libm: the bit-for-bit yardstick."""
    reqs = np.ascontiguousarray(reqs, dtype=abi.SPEC_REQ_DTYPE).reshape(-1)
    out_v = np.asarray(out_v, dtype=np.float64)
    ni, n_points = out_v.shape[0], out_v.shape[1]
    rows = np.zeros((ni, len(reqs), abi.spec_row_doubles(reqs)))
    for r, q in enumerate(reqs):
        log2n, s0, kind, b0, b1 = int(q["log2n"]), int(q["step_from"]), int(q["kind"]), int(q["bin_from"]), int(q["bin_to"])
        if not abi.SPEC_MIN_LOG2N <= log2n <= abi.SPEC_MAX_LOG2N:
            raise ValueError(f"reduce_reference_spectrum: request {r}: log2n {log2n} outside {abi.SPEC_MIN_LOG2N}..{abi.SPEC_MAX_LOG2N}")
        N = 1 << log2n
        half = N // 2
        if not (0 <= s0 and s0 + N <= n_points) or not (0 <= b0 <= b1 <= half) or kind not in (abi.SPEC_BINS, abi.SPEC_DOMINANT) \
                or int(q["window"]) not in (abi.SPEC_RECT, abi.SPEC_HANN):
            raise ValueError(f"reduce_reference_spectrum: request {r}: samples [{s0}, {s0 + N}) outside the run, band [{b0}, {b1}] outside [0, {half}], "
                             f"or unknown kind / window")
        t_re, t_im, w = spectrum_tables(log2n)
        y = _signal_samples(out_v, out_i, q, "reduce_reference_spectrum")[:, s0:s0 + N]
        if int(q["window"]) == abi.SPEC_HANN:
            y = y * w[None, :]
        j = np.arange(N)
        rev = np.zeros(N, np.int64)
        for b in range(log2n):
            rev |= ((j >> b) & 1) << (log2n - 1 - b)
        re_ = np.ascontiguousarray(y[:, rev])  # (slot bitrev(j) holds y_j; bitrev is its own inverse)
        im_ = np.zeros_like(re_)
        for s in range(log2n):
            h = 1 << s
            k = np.arange(h) << (log2n - 1 - s)
            wr, wi = t_re[k][None, None, :], t_im[k][None, None, :]
            re4, im4 = re_.reshape(ni, N // (2 * h), 2, h), im_.reshape(ni, N // (2 * h), 2, h)
            ar, ai, br, bi = re4[:, :, 0, :], im4[:, :, 0, :], re4[:, :, 1, :], im4[:, :, 1, :]
            tr = br * wr - bi * wi
            ti = br * wi + bi * wr
            re_ = np.stack([ar + tr, ar - tr], axis=2).reshape(ni, N)
            im_ = np.stack([ai + ti, ai - ti], axis=2).reshape(ni, N)
        if kind == abi.SPEC_BINS:
            nb = b1 - b0 + 1
            rows[:, r, 0:2 * nb:2] = re_[:, b0:b1 + 1]
            rows[:, r, 1:2 * nb:2] = im_[:, b0:b1 + 1]
            continue
        P = re_[:, :half + 1] * re_[:, :half + 1] + im_[:, :half + 1] * im_[:, :half + 1]
        band = np.where(np.isnan(P[:, b0:b1 + 1]), -1.0, P[:, b0:b1 + 1])  # (`P > best`: a NaN never wins)
        for i in range(ni):
            k = b0 + int(np.argmax(band[i]))  # (first occurrence)
            if not band[i, k - b0] > 0.0:
                rows[i, r, 0] = -1.0
                continue
            rows[i, r, :6] = (k, re_[i, k], im_[i, k], P[i, k - 1] if k >= 1 else -1.0, P[i, k], P[i, k + 1] if k + 1 <= half else -1.0)
    return rows


def derive_timing(spec, rows) -> dict:
    """The values of one timing spec from the rows {k_trig, t_trig, L_trig, k_targ, t_targ, L_targ, n_trig, n_targ} of its
    requests (module text)."""
    def t(row, o):
        return float(row[o + 1]) if row[o] >= 0 else None

    r = rows[0]
    if isinstance(spec, When):
        return {"t": t(r, 3), "level": float(r[5]), "count": int(r[7])}
    if isinstance(spec, Settle):
        ts = [v for v in (t(rows[0], 3), t(rows[1], 3)) if v is not None]
        return {"t": max(ts) if ts else 0.0, "level_lo": float(rows[0][5]), "level_hi": float(rows[1][5])}
    t0, t1 = t(r, 0), t(r, 3)
    d = t1 - t0 if t0 is not None and t1 is not None else None
    if isinstance(spec, Transition):
        return {"t_start": t0, "t_end": t1, "time": d, "level_start": float(r[2]), "level_end": float(r[5])}
    return {"t_trig": t0, "t_targ": t1, "delay": d, "level_trig": float(r[2]), "level_targ": float(r[5]), "count_trig": int(r[6]),
            "count_targ": int(r[7])}


def _signal_samples(out_v: np.ndarray, out_i: Optional[np.ndarray], req, who: str) -> np.ndarray:
    """The signal a request (or an edge of one) names over the whole run, [n_inst][n_points]: column `col` of out_v or out_i,
    minus column `col_ref` if there is one."""
    a = out_i if int(req["signal"]) == 1 else out_v
    if a is None:
        raise ValueError(f"{who}: a request names a current, but there is no out_i")
    a = np.asarray(a, dtype=np.float64)
    x = a[:, :, int(req["col"])]
    return x - a[:, :, int(req["col_ref"])] if int(req["col_ref"]) >= 0 else x


def reduce_reference_timing(out_v: np.ndarray, out_i: Optional[np.ndarray], reqs, dt: float) -> np.ndarray:
    """The definition of spicey_timing_device in numpy, independent of the kernels: out_v [n_inst][n_points][n_v], out_i
    likewise or None, reqs records of abi.TIMING_REQ_DTYPE (step_to / base_to resolved or -1) -> [n_inst][n_req][8] =
    {k_trig, t_trig, L_trig, k_targ, t_targ, L_targ, n_trig, n_targ}.  Every crossing of the window at once, no chunks;
    every field has one value whatever the order."""
    reqs = np.ascontiguousarray(reqs, dtype=abi.TIMING_REQ_DTYPE).reshape(-1)
    out_v = np.asarray(out_v, dtype=np.float64)
    ni, n_points = out_v.shape[0], out_v.shape[1]
    out = np.zeros((ni, len(reqs), 8))

    def level(e, xi, r):
        kind, frac = int(e["level_kind"]), float(e["level"])
        if kind == abi.TIMING_ABS:
            return frac
        b0 = int(e["base_from"])
        b1 = n_points - 1 if int(e["base_to"]) == -1 else int(e["base_to"])
        if not (0 <= b0 <= b1 < n_points):
            raise ValueError(f"reduce_reference_timing: request {r}: base window [{b0}, {b1}] outside the run")
        w = xi[b0:b1 + 1].tolist()
        if kind == abi.TIMING_MINMAX:
            lo = hi = w[0]
            for v in w:  # (the comparisons v < lo, v > hi skip a NaN, like the device's)
                if v < lo:
                    lo = v
                if v > hi:
                    hi = v
        else:
            lo, hi = w[0], w[-1]
        span = hi - lo
        part = frac * span
        return lo + part

    def find(e, xi, L, k0, k1):
        """(k, t, count) of edge e among the crossings in the intervals k0 .. k1 - 1."""
        xa, xb = xi[k0:k1], xi[k0 + 1:k1 + 1]
        hit = np.zeros(len(xa), bool)
        d, n = int(e["dir"]), int(e["n"])
        if d >= 0:
            hit |= (xa < L) & (xb >= L)
        if d <= 0:
            hit |= (xa > L) & (xb <= L)
        ks = np.nonzero(hit)[0]
        m = n - 1 if n >= 1 else len(ks) + n
        if not 0 <= m < len(ks):
            return -1.0, -1.0, float(len(ks))
        k = k0 + int(ks[m])
        a, b = float(xi[k]), float(xi[k + 1])
        return float(k), (float(k) + (L - a) / (b - a)) * dt, float(len(ks))

    for r, q in enumerate(reqs):
        s0 = int(q["step_from"])
        s1 = n_points - 1 if int(q["step_to"]) == -1 else int(q["step_to"])
        if not (0 <= s0 < s1 < n_points):
            raise ValueError(f"reduce_reference_timing: request {r}: window [{s0}, {s1}] outside the run or without an interval")
        x_targ = _signal_samples(out_v, out_i, q["targ"], "reduce_reference_timing")
        x_trig = _signal_samples(out_v, out_i, q["trig"], "reduce_reference_timing") if int(q["has_trig"]) else None
        for i in range(ni):
            row = [-1.0, -1.0, 0.0, -1.0, -1.0, 0.0, 0.0, 0.0]
            k0 = s0
            search = True
            if x_trig is not None:
                L = level(q["trig"], x_trig[i], r)
                row[0], row[1], row[6] = find(q["trig"], x_trig[i], L, s0, s1)
                row[2] = L
                if int(q["targ_from_trig"]):
                    search = row[0] >= 0
                    k0 = int(row[0])
            L = level(q["targ"], x_targ[i], r)
            row[5] = L
            if search:
                row[3], row[4], row[7] = find(q["targ"], x_targ[i], L, k0, s1)
            out[i, r] = row
    return out


def reduce_reference(out_v: np.ndarray, out_i: Optional[np.ndarray], reqs, dt: float) -> np.ndarray:
    """The definition of spicey_measure_device in numpy, independent of the kernels: out_v [n_inst][n_points][n_v], out_i
    likewise or None, reqs records of abi.MEAS_REQ_DTYPE with step_to resolved or -1 -> meas [n_inst][n_req][8].  The sums
    are plain Python sums in step order; everything else has one value whatever the order."""
    reqs = np.ascontiguousarray(reqs, dtype=abi.MEAS_REQ_DTYPE).reshape(-1)
    out_v = np.asarray(out_v, dtype=np.float64)
    ni, n_points = out_v.shape[0], out_v.shape[1]
    meas = np.zeros((ni, len(reqs), 8))
    for r, q in enumerate(reqs):
        x = _signal_samples(out_v, out_i, q, "reduce_reference")
        s0 = int(q["step_from"])
        s1 = n_points - 1 if int(q["step_to"]) == -1 else int(q["step_to"])
        if not (0 <= s0 <= s1 < n_points):
            raise ValueError(f"reduce_reference: request {r}: window [{s0}, {s1}] outside the run")
        x = x[:, s0:s1 + 1]
        for i in range(ni):
            xi = x[i]
            if int(q["kind"]) == abi.MEAS_STATS:
                if np.isnan(xi).any():  # (the comparisons x < m, x > m skip a NaN; numpy's argmin would return it)
                    mn = mx = float(xi[0])
                    kmn = kmx = 0
                    for k, v in enumerate(xi.tolist()):
                        if v < mn:
                            mn, kmn = v, k
                        if v > mx:
                            mx, kmx = v, k
                else:
                    kmn, kmx = int(np.argmin(xi)), int(np.argmax(xi))  # (first occurrence)
                    mn, mx = float(xi[kmn]), float(xi[kmx])
                vals = xi.tolist()
                s = 0.0
                sq = 0.0
                for v in vals:
                    s += v
                    sq += v * v
                meas[i, r] = (mn, mx, s0 + kmn, s0 + kmx, s, sq, vals[0], vals[-1])
            else:
                lv, d = float(q["level"]), int(q["dir"])
                xa, xb = xi[:-1], xi[1:]
                hit = np.zeros(len(xa), bool)
                if d >= 0:
                    hit |= (xa < lv) & (xb >= lv)
                if d <= 0:
                    hit |= (xa > lv) & (xb <= lv)
                ks = np.nonzero(hit)[0]
                if len(ks):
                    t = ((s0 + ks).astype(np.float64) + (lv - xa[ks]) / (xb[ks] - xa[ks])) * dt
                    meas[i, r, :3] = (len(ks), t[0], t[-1])
                else:
                    meas[i, r, :3] = (0.0, -1.0, -1.0)
    return meas


def reduce_reference_power(out_v: np.ndarray, out_i: Optional[np.ndarray], reqs, dt: float) -> np.ndarray:
    """The definition of spicey_power_device in numpy, independent of the kernels: out_v [n_inst][n_points][n_v], out_i
    likewise or None, reqs records of abi.POWER_REQ_DTYPE with step_to resolved or -1 -> [n_inst][n_req][16].  The three sums
    are plain Python sums in step order; everything else has one value whatever the order."""
    reqs = np.ascontiguousarray(reqs, dtype=abi.POWER_REQ_DTYPE).reshape(-1)
    out_v = np.asarray(out_v, dtype=np.float64)
    ni, n_points = out_v.shape[0], out_v.shape[1]
    rows = np.zeros((ni, len(reqs), abi.POWER_ROW))

    def factor(q, pre):
        return _signal_samples(out_v, out_i, {k: q[pre + k] for k in ("signal", "col", "col_ref")}, "reduce_reference_power")

    for r, q in enumerate(reqs):
        s0 = int(q["step_from"])
        s1 = n_points - 1 if int(q["step_to"]) == -1 else int(q["step_to"])
        if not (0 <= s0 <= s1 < n_points) or int(q["neg"]) not in (0, 1):
            raise ValueError(f"reduce_reference_power: request {r}: window [{s0}, {s1}] outside the run, or neg {int(q['neg'])}")
        a, b = factor(q, "a_")[:, s0:s1 + 1], factor(q, "b_")[:, s0:s1 + 1]
        p = a * b
        if int(q["neg"]):
            p = -p
        for i in range(ni):
            pi, ai, bi = p[i].tolist(), a[i].tolist(), b[i].tolist()
            if np.isnan(p[i]).any():  # (the comparisons p < m, p > m skip a NaN; numpy's argmin would return it)
                mn = mx = pi[0]
                kmn = kmx = 0
                for k, v in enumerate(pi):
                    if v < mn:
                        mn, kmn = v, k
                    if v > mx:
                        mx, kmx = v, k
            else:
                kmn, kmx = int(np.argmin(p[i])), int(np.argmax(p[i]))  # (first occurrence)
                mn, mx = pi[kmn], pi[kmx]
            s = saa = sbb = 0.0
            for k in range(len(pi)):
                s += pi[k]
                saa += ai[k] * ai[k]
                sbb += bi[k] * bi[k]
            rows[i, r, :13] = (mn, mx, s0 + kmn, s0 + kmx, s, pi[0], pi[-1], saa, sbb, ai[0], ai[-1], bi[0], bi[-1])
    return rows


def reduce_reference_values(out_v: np.ndarray, out_i: Optional[np.ndarray], reqs, pts, dt: float, timing: Optional[np.ndarray] = None) -> np.ndarray:
    """The definition of spicey_values_device in plain numpy, bit for bit: out_v [n_inst][n_points][n_v], out_i likewise or
    None, reqs records of abi.VAL_REQ_DTYPE (step_to resolved or -1), pts records of abi.VAL_POINT_DTYPE, timing
    [n_inst][n_timing][8] (the rows of the timing pass; needed by find requests) -> [n_inst][n_req][row], row = the longest
    request's, zeros behind a request's own.  No chunks except where a NaN makes them matter: a bucket with one is walked
    in sub-chunks of 256 steps from its own first step, as the device does."""
    reqs = np.ascontiguousarray(reqs, dtype=abi.VAL_REQ_DTYPE).reshape(-1)
    pts = np.ascontiguousarray(pts, dtype=abi.VAL_POINT_DTYPE).reshape(-1)
    out_v = np.asarray(out_v, dtype=np.float64)
    ni, n_points = out_v.shape[0], out_v.shape[1]
    rows = np.zeros((ni, len(reqs), abi.val_row_doubles(reqs)))
    chunk = 256

    def interpolate(y, inst, k, f):
        """{k, f, value, slope} at the points (inst[j], k[j] + f[j]): every operation a numpy operation of its own."""
        y0, y1 = y[inst, k], y[inst, k + 1]
        d = y1 - y0
        return np.stack([k.astype(np.float64), f, np.where(f == 0.0, y0, np.where(f == 1.0, y1, y0 + f * d)), d / dt], axis=-1)

    for r, q in enumerate(reqs):
        kind = int(q["kind"])
        y = _signal_samples(out_v, out_i, q, "reduce_reference_values")
        if kind == abi.VAL_TRACE:
            s0, B = int(q["step_from"]), int(q["buckets"])
            s1 = n_points - 1 if int(q["step_to"]) == -1 else int(q["step_to"])
            if not (0 <= s0 <= s1 < n_points) or not 1 <= B <= min(s1 - s0 + 1, abi.TRACE_MAX_BUCKETS):
                raise ValueError(f"reduce_reference_values: request {r}: window [{s0}, {s1}] outside the run, or {B} buckets")
            lo, hi = trace_buckets(q, n_points)
            out = rows[:, r, :abi.VAL_TRACE_DOUBLES * B].reshape(ni, B, abi.VAL_TRACE_DOUBLES)
            for b in range(B):
                x = y[:, lo[b]:hi[b] + 1]
                kmn, kmx = np.argmin(x, axis=1), np.argmax(x, axis=1)  # (first occurrence)
                for i in np.nonzero(np.isnan(x).any(axis=1))[0]:  # (the comparisons x < m, x > m skip a NaN; argmin would return it)
                    xi = x[i].tolist()
                    part = []
                    for c0 in range(0, len(xi), chunk):
                        mn = mx = xi[c0]
                        a = z = c0
                        for k in range(c0 + 1, min(c0 + chunk, len(xi))):
                            if xi[k] < mn:
                                mn, a = xi[k], k
                            if xi[k] > mx:
                                mx, z = xi[k], k
                        part.append((mn, a, mx, z))
                    mn, a, mx, z = part[0]
                    for pmn, pa, pmx, pz in part[1:]:
                        if pmn < mn:
                            mn, a = pmn, pa
                        if pmx > mx:
                            mx, z = pmx, pz
                    kmn[i], kmx[i] = a, z
                ii = np.arange(ni)
                out[:, b, 0], out[:, b, 1], out[:, b, 2], out[:, b, 3] = x[ii, kmn], lo[b] + kmn, x[ii, kmx], lo[b] + kmx
                out[:, b, 4], out[:, b, 5] = x[:, 0], x[:, -1]
            rows[:, r, :abi.VAL_TRACE_DOUBLES * B] = out.reshape(ni, -1)
        elif kind == abi.VAL_POINTS:
            first, count = int(q["first"]), int(q["count"])
            if n_points < 2 or not (0 <= first and count >= 1 and first + count <= len(pts)):
                raise ValueError(f"reduce_reference_values: request {r}: point run [{first}, {first + count}) outside the table, or a run of one point")
            k, f = pts["k"][first:first + count].astype(np.int64), pts["f"][first:first + count].astype(np.float64)
            if ((k < 0) | (k > n_points - 2) | ~((f >= 0.0) & (f <= 1.0))).any():
                raise ValueError(f"reduce_reference_values: request {r}: a point's k outside [0, {n_points - 2}] or f outside [0, 1]")
            ii = np.repeat(np.arange(ni), count)
            rows[:, r, :abi.VAL_POINT_DOUBLES * count] = interpolate(y, ii, np.tile(k, ni), np.tile(f, ni)).reshape(ni, -1)
        elif kind == abi.VAL_FIND:
            tr = int(q["timing_row"])
            if timing is None or not 0 <= tr < np.asarray(timing).shape[1] or n_points < 2:
                raise ValueError(f"reduce_reference_values: request {r}: timing_row {tr} outside the timing rows given, or a run of one point")
            x = _signal_samples(out_v, out_i, {"signal": q["x_signal"], "col": q["x_col"], "col_ref": q["x_col_ref"]}, "reduce_reference_values")
            kd, L = np.asarray(timing)[:, tr, 3], np.asarray(timing)[:, tr, 5]
            found = (kd >= 0.0) & (kd <= float(n_points - 2))
            rows[:, r, 0] = -1.0
            ii = np.nonzero(found)[0]
            if len(ii):
                k = kd[ii].astype(np.int64)
                a, b = x[ii, k], x[ii, k + 1]
                with np.errstate(all="ignore"):
                    f = (L[ii] - a) / (b - a)
                    rows[ii, r, :4] = interpolate(y, ii, k, f)
        else:
            raise ValueError(f"reduce_reference_values: request {r}: unknown kind {kind}")
    return rows


def reduce_reference_fourier(out_v: np.ndarray, out_i: Optional[np.ndarray], reqs, dt: float) -> np.ndarray:
    """The definition of spicey_fourier_device in numpy, independent of the kernels: out_v [n_inst][n_points][n_v], out_i
    likewise or None, reqs records of abi.FOUR_REQ_DTYPE with step_to resolved or -1 -> [n_inst][n_req][1 + 2 max n_harm],
    {C0, C1, S1, ...} and zeros behind a request's own 1 + 2 n_harm.  The twiddle argument is formed by the same three
    operations as the library's (r = float(h s) (f0 dt); r -= floor(r); a = 2 pi r), cos / sin are numpy's; every product is
    rounded on its own and every sum runs over the window in step order, one addition after the other from 0.0
    (np.add.accumulate: no pairwise regrouping) — no chunks."""
    reqs = np.ascontiguousarray(reqs, dtype=abi.FOUR_REQ_DTYPE).reshape(-1)
    out_v = np.asarray(out_v, dtype=np.float64)
    ni, n_points = out_v.shape[0], out_v.shape[1]
    width = 1 + 2 * int(reqs["n_harm"].max()) if len(reqs) else 1
    rows = np.zeros((ni, len(reqs), width))
    tw_cache: Dict[tuple, tuple] = {}
    for r, q in enumerate(reqs):
        x = _signal_samples(out_v, out_i, q, "reduce_reference_fourier")
        s0, H, f0 = int(q["step_from"]), int(q["n_harm"]), float(q["f0"])
        s1 = n_points - 1 if int(q["step_to"]) == -1 else int(q["step_to"])
        if not (0 <= s0 < s1 < n_points) or not 1 <= H <= abi.FOUR_MAX_HARM:
            raise ValueError(f"reduce_reference_fourier: request {r}: window [{s0}, {s1}) outside the run, or n_harm {H}")
        x = x[:, s0:s1]
        key = (f0, s0, s1, H)
        if key not in tw_cache:
            hs = np.arange(1, H + 1, dtype=np.int64)[:, None] * np.arange(s0, s1, dtype=np.int64)[None, :]
            t = hs.astype(np.float64) * (f0 * dt)
            t = t - np.floor(t)
            ang = (2.0 * np.pi) * t
            tw_cache[key] = (np.cos(ang), np.sin(ang))
        c, sn = tw_cache[key]
        zero = np.zeros(x.shape[:1] + (1,))
        rows[:, r, 0] = np.add.accumulate(np.concatenate([zero, x], axis=1), axis=1)[:, -1]
        z3 = np.zeros((ni, H, 1))
        rows[:, r, 1:2 * H + 1:2] = np.add.accumulate(np.concatenate([z3, x[:, None, :] * c[None]], axis=2), axis=2)[:, :, -1]
        rows[:, r, 2:2 * H + 2:2] = np.add.accumulate(np.concatenate([z3, x[:, None, :] * sn[None]], axis=2), axis=2)[:, :, -1]
    return rows


def backend_reduce(be, flat: abi.FlatCircuit, steps: int, dt: float, src: np.ndarray, reqs: np.ndarray, freqs: np.ndarray, treqs: np.ndarray,
                   need_i: bool, sreqs: Sequence = (), preqs: Sequence = (), vreqs: Sequence = (), pts: Sequence = ()) -> dict:
    """With a values list the backend's run_reduced (every list at once); without one, as ever, the backend's run_measure_power, run_measure_spectrum, run_measure_timing, run_measure_fourier or run_measure — the
    first whose own list is not empty — or for a backend without that method its run followed by the numpy reductions of that
    method's passes."""
    method, args = ("run_reduced", (reqs, freqs, treqs, sreqs, preqs, vreqs, pts)) if len(vreqs) else \
        ("run_measure_power", (reqs, freqs, treqs, sreqs, preqs)) if len(preqs) else \
        ("run_measure_spectrum", (reqs, freqs, treqs, sreqs)) if len(sreqs) else ("run_measure_timing", (reqs, freqs, treqs)) if len(treqs) else \
        ("run_measure_fourier", (reqs, freqs)) if len(freqs) else ("run_measure", (reqs,))
    if hasattr(be, method):
        return getattr(be, method)(flat, steps, dt, src, *args)
    res = be.run(flat, steps, dt, src, want_currents=need_i)
    if res["status"] == abi.OK or (res["status"] == abi.ERR_SINGULAR and res.get("partial")):
        for key, fn, lst in zip(("meas", "four", "timing", "spec", "power"),
                                (reduce_reference, reduce_reference_fourier, reduce_reference_timing, reduce_reference_spectrum, reduce_reference_power), args):
            res[key] = fn(res["out_v"], res.get("out_i"), lst, dt)  # (an empty list: [n_inst][0][8], [n_inst][0][1])
        if len(vreqs):
            res["values"] = reduce_reference_values(res["out_v"], res.get("out_i"), vreqs, pts, dt, res["timing"])
    return res


def _backend(backend, exact_order: bool, device: int, diagnostics: bool, who: str):
    if exact_order and backend is not None:
        raise ValueError(f"{who}: pass either backend= or exact_order=True, not both")
    if backend is not None:
        return backend
    from .lib import HipBackend  # fails loudly if the extension is missing

    return HipBackend(device=device, diagnostics=1 if diagnostics else 0, interpreter=3 if exact_order else 0)


def measureTRAN(ckt: ParsedCircuit, measures: Dict[str, object], *, exact_order: bool = False, device: int = 0, backend=None) -> Optional[dict]:
    """The transient of `ckt` reduced to {name: {...}} for measures = {name: stats(...) | cross(...) | fourier(...) | when(...) | delay(...) | spectrum(...) | dominant(...) | power(...) | efficiency(...) | trace(...) | sample(...) | find(...) | ...} (module text).  None
    without a .tran card; SingularMatrixError and the circuit's state write-back exactly as simulateTRAN; exact_order=True
    runs the reference-order engine."""
    be = _backend(backend, exact_order, device, True, "measureTRAN")
    tran = ckt.analyses.get("tran")
    if not tran:
        return None
    dt, steps = abi.computeEffectiveTimeStep(tran["dt"], tran["tstop"])
    plan = _Plan(ckt, measures, dt, steps)
    flat = plan.flatten(ckt)
    src = abi.source_table(ckt, dt, steps)
    res = plan.run(be, flat, steps, dt, src)
    if res["status"] == abi.ERR_SINGULAR:
        raise SingularMatrixError(res.get("detail", ""))
    if res["status"] != abi.OK:
        raise RuntimeError(res.get("detail", f"spicey native error {res['status']}"))
    write_state(ckt, res["state"], 0)
    return plan.values(res, 0, dt)


def measureTRANBatch(ckts: Sequence[ParsedCircuit], measures: Dict[str, object], *, exact_order: bool = False, diagnostics: bool = True,
                     device: int = 0, max_instances: int = 4096, backend=None) -> List[Optional[object]]:
    """measureTRAN for many circuits in as few launches as simulateTRANBatch would make (spicey_amd/batch.py): circuits that
    share topology, measured columns, windows, dt and step count are the instances of one handle, with the measured nodes as
    the recorded nodes; groups above max_instances are split; instances a failing workgroup mate stopped run again.  Slot i
    is measureTRAN(ckts[i], measures)'s dict, None without .tran, or — returned, not raised, with the circuit's state left
    alone — its SingularMatrixError."""
    seen = set()
    for c in ckts:
        if id(c) in seen:
            raise ValueError("measureTRANBatch: the same circuit object appears twice (its state would be written twice)")
        seen.add(id(c))
    be = _backend(backend, exact_order, device, diagnostics, "measureTRANBatch")
    out: List[Optional[object]] = [None] * len(ckts)
    plans: Dict[int, _Plan] = {}

    def plan_of(c: ParsedCircuit) -> _Plan:
        if id(c) not in plans:
            tran = c.analyses["tran"]
            dt, steps = abi.computeEffectiveTimeStep(tran["dt"], tran["tstop"])
            plans[id(c)] = _Plan(c, measures, dt, steps)
        return plans[id(c)]

    # (names resolve per circuit: two circuits of one topology may call its elements differently — the request records
    # are part of the group's key, so one launch has one request table)
    launches = group_launches(ckts, max_instances, lambda c: plan_of(c).flatten(c), lambda c, dt, steps: plan_of(c).key())
    for idx in launches:
        plan = plan_of(ckts[idx[0]])

        def result(i, flat_i, dt, steps, res, j, sk):
            write_state(ckts[i], res["state"], j)
            return plan_of(ckts[i]).values(res, j, dt)

        run_launch(lambda flat, steps, dt, src: plan.run(be, flat, steps, dt, src), ckts, idx, out, diagnostics,
                   lambda c: plan_of(c).flatten(c), result, "measureTRANBatch")
    return out
