"""measureAC() / measureACBatch(): a few numbers per circuit instead of every node's and element's response.

simulateAC returns the whole sweep; a tolerance or corner sweep of a filter is usually run for the -3 dB corner, the peak
and the phase at unity gain.  Here the sweep's complex results stay on the device and a reduction pass
(spicey_ac_run_measure, include/spicey_hip.h) brings back 8 doubles per (circuit, measure).  Only the measured nodes are
recorded (SpiceyDesc.out_nodes) and element currents only if a measure names one.

Specs
    extrema("v(out)", what="mag")            min, max, f_min, f_max, H_min, H_max (+ db_min, db_max, phase_min_deg,
                                             phase_max_deg for what="mag", whose min / max are magnitudes)
    at("v(out)/v(in)", 1e3)                  f, H, mag, db, phase_deg at the nearest listed frequency (a tie: the higher)
    fcross("v(out)/v(in)", 0.5 ** 0.5)       count, f, H, mag, db, phase_deg, f_lo, f_hi — where the measured quantity
                                             crosses the level; rel=True: level times the quantity at the window's start
`signal` is "v(a)", "v(a,b)" (= v(a) - v(b), one rounded subtraction per part), "i(R1)" (the element current simulateAC
records under that name) or a quotient of two of them.  Names resolve case-insensitively like measure.py's; a name that
several elements share is an error.  `what` is the real quantity looked at: "mag" (the device works on |H|^2 — no sqrt, log
or atan2 runs there), "re" or "im".

Windows.  f_from / f_to (Hz, None = the sweep's first / last point) select the frequency indices with f_from <= freqs[k]
<= f_to; an empty or non-contiguous set is a ValueError.

Derived values (on the host).  extrema / at: H is the complex sample at the extreme; mag = sqrt(|H|^2), db = 20 log10(mag),
phases by atan2 in degrees.  fcross: the device names the bracket (k, k + 1) of the first (which="first") or last crossing
and its two samples; with q = the measured quantity of each and thr the threshold the device used,
t = (thr - q_k) / (q_k+1 - q_k), f = f_k (f_k+1 / f_k)^t for interp="log" (the default for a `dec` card) or f_k + t (f_k+1 -
f_k) for "lin", clamped to the bracket, H = H_k + t (H_k+1 - H_k), mag = |H|.  For what="mag" the level is a magnitude (the
host sends level^2; db=True converts 10^(level / 20) first).  Without a crossing every value but `count` is None.

reduce_ac_reference() is the same definition in plain numpy; it is what the tests compare the device with, and what runs
behind a backend that has no run_ac_measure (backend.run_ac, then reduce_ac_reference: the CPU oracle works unchanged).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .ac import buildFrequencyArray
from .ac_batch import ac_group_launches, batch_backend, launch_status, slot_error, stacked
from .measure import _parse_signal
from .netlist import ParsedCircuit

_DIRS = {"rise": 1, "fall": -1, "either": 0}
_WHAT = {"mag": abi.AC_WHAT_MAG2, "re": abi.AC_WHAT_RE, "im": abi.AC_WHAT_IM}
_WHICH = {"first": 0, "last": 1}


@dataclass(frozen=True)
class Extrema:
    signal: str
    what: str = "mag"
    f_from: Optional[float] = None
    f_to: Optional[float] = None


@dataclass(frozen=True)
class At:
    signal: str
    f: float


@dataclass(frozen=True)
class FCross:
    signal: str
    level: float
    what: str = "mag"
    dir: int = -1
    which: int = 0
    rel: bool = False
    db: bool = False
    interp: Optional[str] = None
    f_from: Optional[float] = None
    f_to: Optional[float] = None


Spec = (Extrema, At, FCross)


def _what(who: str, what: str) -> str:
    if what not in _WHAT:
        raise ValueError(f"{who}: what must be 'mag', 're' or 'im', got {what!r}")
    return what


def extrema(signal: str, what: str = "mag", f_from: Optional[float] = None, f_to: Optional[float] = None) -> Extrema:
    return Extrema(str(signal), _what("extrema", what), f_from, f_to)


def at(signal: str, f: float) -> At:
    return At(str(signal), float(f))


def fcross(signal: str, level: float, what: str = "mag", dir="fall", which="first", rel: bool = False, db: bool = False,
           interp: Optional[str] = None, f_from: Optional[float] = None, f_to: Optional[float] = None) -> FCross:
    if dir not in _DIRS:
        raise ValueError(f"fcross: dir must be 'rise', 'fall' or 'either', got {dir!r}")
    if which not in _WHICH:
        raise ValueError(f"fcross: which must be 'first' or 'last', got {which!r}")
    if interp not in (None, "log", "lin"):
        raise ValueError(f"fcross: interp must be 'log' or 'lin', got {interp!r}")
    if db and what != "mag":
        raise ValueError("fcross: db=True needs what='mag'")
    return FCross(str(signal), float(level), _what("fcross", what), _DIRS[dir], _WHICH[which], bool(rel), bool(db), interp, f_from, f_to)


def make_ac_reqs(rows: Sequence[tuple]) -> np.ndarray:
    """Request records (abi.AC_MEAS_REQ_DTYPE) from tuples (num_signal, num_col, num_col_ref, den_signal, den_col, den_col_ref,
    what, kind, k_from, k_to, level, dir, which, rel)."""
    a = np.zeros(len(rows), abi.AC_MEAS_REQ_DTYPE)
    for k, r in enumerate(rows):
        a[k] = tuple(r) + (0,)
    return a


def _ac_element_names(ckt: ParsedCircuit) -> List[str]:
    # simulateAC's recording order (R, C, L, V): the columns of out_i
    return [e.name for e in ckt.R] + [e.name for e in ckt.C] + [e.name for e in ckt.L] + [e.name for e in ckt.V]


def _split_quotient(text: str) -> List[str]:
    parts, depth, cur = [], 0, ""
    for ch in text:
        if ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
        if ch == "/" and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    return parts + [cur]


def parse_ac_signal(ckt: ParsedCircuit, text: str) -> List[Tuple[int, int, int]]:
    """[numerator] or [numerator, denominator], each (signal, a, b) as measure._parse_signal gives them."""
    parts = _split_quotient(text)
    if len(parts) > 2:
        raise ValueError(f"measure: {text!r}: at most one quotient (a / b)")
    names = _ac_element_names(ckt)
    return [_parse_signal(ckt, p, names) for p in parts]


def freq_window(freqs: np.ndarray, f_from: Optional[float], f_to: Optional[float], name: str) -> Tuple[int, int]:
    lo = -math.inf if f_from is None else float(f_from)
    hi = math.inf if f_to is None else float(f_to)
    ks = np.nonzero((freqs >= lo) & (freqs <= hi))[0]
    if not len(ks):
        raise ValueError(f"measure {name!r}: the window is empty (no listed frequency in [{lo}, {hi}])")
    if int(ks[-1]) - int(ks[0]) + 1 != len(ks):
        raise ValueError(f"measure {name!r}: the window's frequencies are not contiguous in the sweep")
    return int(ks[0]), int(ks[-1])


def nearest_index(freqs: np.ndarray, f: float) -> int:
    """The listed frequency nearest to f, a tie going to the higher one."""
    d = np.abs(freqs - f)
    ties = np.nonzero(d == d.min())[0]
    return int(ties[np.argmax(freqs[ties])])


class _Plan:
    """A circuit's measures resolved: the recorded nodes, whether currents are needed, the request records."""

    def __init__(self, ckt: ParsedCircuit, measures: Dict[str, object], freqs: np.ndarray, mode: str):
        if not measures:
            raise ValueError("measure: no measures given")
        if not len(freqs):
            raise ValueError("measure: the sweep has no frequencies")
        parsed = []
        for name, spec in measures.items():
            if not isinstance(spec, Spec):
                raise TypeError(f"measure {name!r}: expected extrema(...), at(...) or fcross(...), got {type(spec).__name__}")
            parsed.append((name, spec, parse_ac_signal(ckt, spec.signal)))
        terms = [t for _, _, ts in parsed for t in ts]
        nodes = sorted({n for sig, a, b in terms if sig == 0 for n in (a, b) if n != 0})
        self.need_i = any(sig == 1 for sig, _, _ in terms)
        # (a device descriptor records at least one node; with current measures only, the first one)
        self.out_nodes = nodes if nodes else [1]
        col = {n: c for c, n in enumerate(self.out_nodes)}

        def cols(t):
            sig, a, b = t
            return (0, col[a], col[b] if b else -1) if sig == 0 else (1, a, -1)

        self.freqs = freqs
        self.mode = mode
        self.names, self.specs, rows = [], [], []
        for name, spec, ts in parsed:
            num = cols(ts[0])
            den = cols(ts[1]) if len(ts) > 1 else (-1, 0, 0)
            if isinstance(spec, At):
                k = nearest_index(freqs, spec.f)
                rows.append(num + den + (abi.AC_WHAT_MAG2, abi.AC_MEAS_EXTREMA, k, k, 0.0, 0, 0, 0))
            elif isinstance(spec, Extrema):
                k0, k1 = freq_window(freqs, spec.f_from, spec.f_to, name)
                rows.append(num + den + (_WHAT[spec.what], abi.AC_MEAS_EXTREMA, k0, k1, 0.0, 0, 0, 0))
            else:
                k0, k1 = freq_window(freqs, spec.f_from, spec.f_to, name)
                lv = 10.0 ** (spec.level / 20.0) if spec.db else spec.level
                if spec.what == "mag":
                    lv = lv * lv
                rows.append(num + den + (_WHAT[spec.what], abi.AC_MEAS_CROSS, k0, k1, lv, spec.dir, spec.which, int(spec.rel)))
            self.names.append(name)
            self.specs.append(spec)
        self.reqs = make_ac_reqs(rows)

    def flatten(self, ckt: ParsedCircuit) -> abi.FlatCircuit:
        flat = abi.flatten(ckt)
        flat.out_nodes = np.ascontiguousarray(self.out_nodes, dtype=np.int32)
        return flat

    def values(self, meas: np.ndarray) -> Dict[str, dict]:
        """meas [n_req][8] of one instance -> {name: {...}}."""
        return {name: derive_ac(self.specs[k], self.reqs[k], meas[k], self.freqs, self.mode) for k, name in enumerate(self.names)}


def _db(mag: float) -> float:
    return 20.0 * math.log10(mag) if mag > 0.0 else (-math.inf if mag == 0.0 else math.nan)


def _deg(z: complex) -> float:
    return math.degrees(math.atan2(z.imag, z.real))


def _q(z: complex, what: int) -> float:
    return z.real * z.real + z.imag * z.imag if what == abi.AC_WHAT_MAG2 else z.real if what == abi.AC_WHAT_RE else z.imag


def derive_ac(spec, req, m, freqs: np.ndarray, mode: str = "dec") -> dict:
    """The values of one measure from its 8 doubles (module text)."""
    m = [float(v) for v in m]
    if isinstance(spec, At):
        h = complex(m[4], m[5])
        mag = math.sqrt(m[0])
        return {"f": float(freqs[int(m[2])]), "H": h, "mag": mag, "db": _db(mag), "phase_deg": _deg(h)}
    if isinstance(spec, Extrema):
        hn, hx = complex(m[4], m[5]), complex(m[6], m[7])
        res = {"min": m[0], "max": m[1], "f_min": float(freqs[int(m[2])]), "f_max": float(freqs[int(m[3])]), "H_min": hn, "H_max": hx}
        if spec.what == "mag":
            res["min"], res["max"] = math.sqrt(m[0]), math.sqrt(m[1])
            res.update(db_min=_db(res["min"]), db_max=_db(res["max"]), phase_min_deg=_deg(hn), phase_max_deg=_deg(hx))
        return res
    count = int(m[0])
    if count == 0:
        return {"count": 0, "f": None, "H": None, "mag": None, "db": None, "phase_deg": None, "f_lo": None, "f_hi": None}
    k = int(m[2]) if spec.which else int(m[1])
    ha, hb, thr = complex(m[3], m[4]), complex(m[5], m[6]), m[7]
    what = int(req["what"])
    qa, qb = _q(ha, what), _q(hb, what)
    t = (thr - qa) / (qb - qa)
    f_lo, f_hi = float(freqs[k]), float(freqs[k + 1])
    interp = spec.interp or ("log" if mode == "dec" else "lin")
    f = f_lo * (f_hi / f_lo) ** t if interp == "log" else f_lo + t * (f_hi - f_lo)
    f = min(max(f, min(f_lo, f_hi)), max(f_lo, f_hi))
    h = ha + t * (hb - ha)
    mag = abs(h)
    return {"count": count, "f": f, "H": h, "mag": mag, "db": _db(mag), "phase_deg": _deg(h), "f_lo": f_lo, "f_hi": f_hi}


def reduce_ac_reference(out_v: np.ndarray, out_i: Optional[np.ndarray], reqs) -> np.ndarray:
    """The definition of spicey_ac_measure_device in numpy, independent of the kernel: out_v complex [n_inst][n_freq][n_v],
    out_i likewise or None, reqs records of abi.AC_MEAS_REQ_DTYPE with k_to resolved or -1 -> meas [n_inst][n_req][8].  Every
    product, sum and quotient is one numpy operation, rounded on its own."""
    reqs = np.ascontiguousarray(reqs, dtype=abi.AC_MEAS_REQ_DTYPE).reshape(-1)
    out_v = np.asarray(out_v, dtype=np.complex128)
    out_i = np.asarray(out_i, dtype=np.complex128) if out_i is not None else None
    ni, nf = out_v.shape[0], out_v.shape[1]
    meas = np.zeros((ni, len(reqs), 8))

    def term(signal, col, col_ref):
        a = out_i if signal == 1 else out_v
        if a is None:
            raise ValueError("reduce_ac_reference: a request names a current, but there is no out_i")
        re, im = a[:, :, col].real, a[:, :, col].imag
        if col_ref >= 0:
            re, im = re - a[:, :, col_ref].real, im - a[:, :, col_ref].imag
        return re, im

    for r, q in enumerate(reqs):
        k0 = int(q["k_from"])
        k1 = nf - 1 if int(q["k_to"]) == -1 else int(q["k_to"])
        if not (0 <= k0 <= k1 < nf):
            raise ValueError(f"reduce_ac_reference: request {r}: window [{k0}, {k1}] outside the sweep")
        re, im = term(int(q["num_signal"]), int(q["num_col"]), int(q["num_col_ref"]))
        if int(q["den_signal"]) >= 0:
            bre, bim = term(int(q["den_signal"]), int(q["den_col"]), int(q["den_col_ref"]))
            with np.errstate(all="ignore"):
                d = bre * bre + bim * bim
                re, im = (re * bre + im * bim) / d, (im * bre - re * bim) / d
        what = int(q["what"])
        with np.errstate(all="ignore"):
            x = re * re + im * im if what == abi.AC_WHAT_MAG2 else re if what == abi.AC_WHAT_RE else im
        for i in range(ni):
            xi = x[i, k0:k1 + 1]
            if int(q["kind"]) == abi.AC_MEAS_EXTREMA:
                # m = x_0, then x < m / x > m in ascending k: first occurrence; a NaN never replaces, a NaN x_0 stays
                mn = mx = float(xi[0])
                kmn = kmx = 0
                if np.isnan(xi).any():
                    for k, v in enumerate(xi.tolist()):
                        if v < mn:
                            mn, kmn = v, k
                        if v > mx:
                            mx, kmx = v, k
                else:
                    kmn, kmx = int(np.argmin(xi)), int(np.argmax(xi))
                    mn, mx = float(xi[kmn]), float(xi[kmx])
                kmn, kmx = k0 + kmn, k0 + kmx
                meas[i, r] = (mn, mx, kmn, kmx, re[i, kmn], im[i, kmn], re[i, kmx], im[i, kmx])
            else:
                with np.errstate(all="ignore"):
                    thr = float(np.float64(q["level"]) * xi[0]) if int(q["rel"]) else float(q["level"])
                    d = int(q["dir"])
                    xa, xb = xi[:-1], xi[1:]
                    hit = np.zeros(len(xa), bool)
                    if d >= 0:
                        hit |= (xa < thr) & (xb >= thr)
                    if d <= 0:
                        hit |= (xa > thr) & (xb <= thr)
                ks = np.nonzero(hit)[0]
                if len(ks):
                    k = k0 + int(ks[-1] if int(q["which"]) else ks[0])
                    meas[i, r] = (len(ks), k0 + ks[0], k0 + ks[-1], re[i, k], im[i, k], re[i, k + 1], im[i, k + 1], thr)
                else:
                    meas[i, r] = (0.0, -1.0, -1.0, 0.0, 0.0, 0.0, 0.0, thr)
    return meas


def backend_ac_measure(be, flat: abi.FlatCircuit, freqs: np.ndarray, vph: np.ndarray, reqs: np.ndarray, need_i: bool) -> dict:
    """The backend's run_ac_measure, or for a backend without one its run_ac followed by reduce_ac_reference (a backend that
    returned every node gets the recorded columns selected)."""
    if hasattr(be, "run_ac_measure"):
        return be.run_ac_measure(flat, freqs, vph, reqs)
    res = be.run_ac(flat, freqs, vph, want_currents=need_i)
    if res.get("out_v") is not None:
        out_v = np.asarray(res["out_v"])
        if flat.out_nodes is not None and len(flat.out_nodes) and out_v.shape[2] == flat.n_nodes != flat.n_out:
            out_v = out_v[:, :, np.asarray(flat.out_nodes) - 1]
        res["meas"] = reduce_ac_reference(out_v, res.get("out_i") if need_i else None, reqs)
    return res


def _card(ckt: ParsedCircuit):
    ac = ckt.analyses.get("ac")
    if not ac:
        return None, None
    return np.asarray(buildFrequencyArray(ac["mode"], ac["N"], ac["f1"], ac["f2"]), dtype=np.float64), ac["mode"]


def measureAC(ckt: ParsedCircuit, measures: Dict[str, object], *, exact_order: bool = False, device: int = 0, backend=None) -> Optional[dict]:
    """The AC sweep of `ckt` reduced to {name: {...}} for measures = {name: extrema(...) | at(...) | fcross(...)} (module
    text).  None without a .ac card; the errors of simulateAC, raised when the sweep fails at ANY frequency (inside a
    measure's window or not); exact_order=True runs the reference-order engine."""
    out = measureACBatch([ckt], measures, exact_order=exact_order, device=device, backend=backend)[0]
    if isinstance(out, Exception):
        raise out
    return out


def measureACBatch(ckts: Sequence[ParsedCircuit], measures: Dict[str, object], *, exact_order: bool = False, device: int = 0,
                   max_instances: int = 4096, max_result_bytes: int = 1 << 30, backend=None) -> List[Optional[object]]:
    """measureAC for many circuits in as few launches as simulateACBatch would make (spicey_amd/ac_batch.py): circuits that
    share topology, measured columns, frequency list and request table are the instances of one handle, with the measured
    nodes as the recorded nodes.  Slot i is measureAC(ckts[i], measures)'s dict, None without .ac, or — returned, not raised —
    the error its sweep ends in."""
    be = batch_backend(backend, exact_order, device, "measureACBatch")
    out: List[Optional[object]] = [None] * len(ckts)
    plans: Dict[int, _Plan] = {}

    def plan_of(c: ParsedCircuit) -> _Plan:
        if id(c) not in plans:
            freqs, mode = _card(c)
            plans[id(c)] = _Plan(c, measures, freqs, mode)
        return plans[id(c)]

    for c in ckts:  # (names and windows are judged for every circuit before anything runs)
        if c.analyses.get("ac"):
            plan_of(c)
    # (names resolve per circuit: the request records are part of the group's key, so one launch has one request table)
    launches = ac_group_launches(ckts, out, max_instances, max_result_bytes, lambda c: plan_of(c).flatten(c),
                                 lambda flat, nf: len(measures) * 64, lambda c, f: plan_of(c).reqs.tobytes())
    for idx, freqs in launches:
        plan = plan_of(ckts[idx[0]])
        flat, vph = stacked(ckts, idx, lambda c: plan_of(c).flatten(c))
        res = backend_ac_measure(be, flat, freqs, vph, plan.reqs, plan.need_i)
        ist = launch_status(res, len(idx), "measureACBatch")
        n_bad = int(np.count_nonzero(ist))
        for j, i in enumerate(idx):
            if int(ist[j]) != 0:
                out[i] = slot_error(int(ist[j]), res.get("detail", "") if n_bad == 1 else "")
            else:
                out[i] = plan_of(ckts[i]).values(res["meas"][j])
    return out
