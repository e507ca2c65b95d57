"""simulateSens() / simulateSensBatch(): first-order AC sensitivities and tolerance bounds of the small-signal circuit.

How the response moves when an element value moves — SPICE's .sens and worst-case analysis — from TWO sweeps of the AC engine
instead of 2 nE + 1: the plain sweep D and the sweep X with every source phasor at zero and a unit current injected into the
output pair (spicey_ac_run_sens, include/spicey_hip.h).  The AC matrix of R, C, L and V is complex symmetric, so X is the
adjoint solution (DESIGN.md "AC sensitivities"): with out = v(p) - v(n) and Y_e the admittance of element e,

    d out / d Y_e = - dx_e dd_e              dx_e, dd_e: the voltage across e in X and in D

and with the recorded currents i = Y dv, prod = i_X(e) i_D(e) and w = 2 pi f the absolute sensitivity S_e = p_e d out / d p_e is

    R: R prod          C: j prod / (w C)          L: j prod (w L)

The relative ones are S_e / H with H = out of sweep D: m_e = Re = d ln|H| / d ln p_e and phi_e = Im = d arg H / d ln p_e (radians).
H = out / V_in differs from out by a constant, so these are the sensitivities of the transfer function as well.  Both sweeps
stay on the device; a reduction pass brings back 6 doubles per frequency and 4 per element (plus, with full=True, 2 per
frequency and element).  Diodes and switches take no part, as in simulateAC.

    simulateSens(ckt, output="v(out)" | "v(a,b)", tol=None | float | dict, freqs=None, f_from=None, f_to=None, full=False)

tol is a RELATIVE tolerance per element (0.01 = 1 %): None is 1.0 for every element, so that the sums are per unit relative
change; a float holds for every element; a dict maps element names (case-insensitive) to tolerances, with the kind keys "R",
"C", "L" as defaults for the elements it does not name (an element neither named nor covered by its kind's key has tolerance
0).  freqs defaults to the .ac card's list (None is returned without either); f_from / f_to select the window the peaks are
searched in.  The result:

    freqs, h                                the sweep's frequencies in Hz, the complex output of sweep D
    mag_wc, mag_sigma                       sum_e t_e |m_e| and sqrt(sum_e (t_e m_e)^2): the worst-case and the root-sum-square
                                            relative change of |H| per frequency, first order
    mag_wc_db                               20 log10(1 + mag_wc)
    phase_wc_deg, phase_sigma_deg           the same for arg H, in degrees
    band                                    (first, last) frequency of the window
    elements                                {name: {kind, value, tol, mag_peak, f_mag_peak, phase_peak_deg, f_phase_peak}}: the
                                            m_e (phi_e) of largest magnitude over the window and where it is, ordered by
                                            |mag_peak| tol, largest first
    mag_sens, phase_sens_deg                with full=True: {name: [n_freq]}, m_e and phi_e (degrees) at every frequency

simulateSensBatch groups, splits and reports per-slot errors exactly like simulateACBatch.  reduce_reference_sens() is the
same definition in plain numpy; it is what the tests compare the device with.  The reference-order engine has no injection:
exact_order=True raises.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .ac_batch import ac_group_launches, batch_backend, launch_status, slot_error, stacked
from .ac_measure import freq_window
from .measure import _parse_signal
from .netlist import ParsedCircuit
from .noise import _freqs_of

LANES = 64
TWO_PI = 2 * 3.141592653589793  # the engine's constant (ac_exec.h)


def _lane_sums(term: np.ndarray) -> np.ndarray:
    """term [n_inst][n_freq][nE] -> [n_inst][n_freq]: lane l adds the elements l, l + 64, ... in ascending order to +0.0, the 64
    partials meet by s[l] += s[l + stride] for stride = 32 .. 1."""
    ni, nf, nE = term.shape
    groups = (nE + LANES - 1) // LANES
    pad = np.zeros((ni, nf, groups * LANES))
    pad[:, :, :nE] = term
    pad = pad.reshape(ni, nf, groups, LANES)
    s = np.zeros((ni, nf, LANES))
    for g in range(groups):
        s = s + pad[:, :, g, :]  # (a lane past the last element adds +0.0: no change to a sum that is >= 0 or NaN)
    stride = LANES // 2
    while stride:
        s[:, :, :stride] = s[:, :, :stride] + s[:, :, stride:2 * stride]
        stride //= 2
    return s[:, :, 0]


def reduce_reference_sens(out_v: np.ndarray, out_i_dir: np.ndarray, out_i_adj: np.ndarray, R: np.ndarray, Cv: np.ndarray, Lv: np.ndarray, tol: np.ndarray,
                          freqs: np.ndarray, out_p: int, out_n: int, k_from: int = 0, k_to: int = -1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The definition of spicey_ac_sens_device in numpy, independent of the kernels: out_v complex [n_inst][n_freq][n_v] and
    out_i_dir complex [n_inst][n_freq][n_i] of the plain sweep, out_i_adj likewise of the injected one (the first nR + nC + nL
    columns are the elements, R then C then L), R / Cv / Lv [n_inst][n<kind>], tol [nE] -> (spec [n_inst][n_freq][6], peak
    [n_inst][nE][4], full [n_inst][n_freq][nE][2]).  Every product, sum and quotient is one numpy operation, rounded on its own,
    in the order of the module text and of DESIGN.md: the complex product, the kind's factor, H by one subtraction per part,
    the two quotients by |H|^2, the lane sums and their tree, the peak by a strict comparison of magnitudes in ascending k."""
    out_v = np.asarray(out_v, dtype=np.complex128)
    x = np.asarray(out_i_adj, dtype=np.complex128)
    y = np.asarray(out_i_dir, dtype=np.complex128)
    R, Cv, Lv = (np.asarray(a, dtype=np.float64).reshape(x.shape[0], -1) for a in (R, Cv, Lv))
    tol = np.asarray(tol, dtype=np.float64).reshape(-1)
    freqs = np.asarray(freqs, dtype=np.float64)
    ni, nf = x.shape[0], x.shape[1]
    nR, nC, nL = R.shape[1], Cv.shape[1], Lv.shape[1]
    nE = nR + nC + nL
    k1 = nf - 1 if k_to == -1 else int(k_to)
    k0 = int(k_from)
    if not (0 <= k0 <= k1 < nf) or out_p == out_n or nE < 1 or nE > x.shape[2] or len(tol) != nE or not (np.isfinite(tol).all() and (tol >= 0).all()):
        raise ValueError("reduce_reference_sens: bad request")
    xr, xi, yr, yi = x[:, :, :nE].real, x[:, :, :nE].imag, y[:, :, :nE].real, y[:, :, :nE].imag
    with np.errstate(all="ignore"):
        pr = xr * yr - xi * yi
        pi = xr * yi + xi * yr
        w = np.float64(TWO_PI) * freqs
        sr, si = np.zeros((ni, nf, nE)), np.zeros((ni, nf, nE))
        a, b = nR, nR + nC
        sr[:, :, :a] = R[:, None, :] * pr[:, :, :a]
        si[:, :, :a] = R[:, None, :] * pi[:, :, :a]
        q = w[None, :, None] * Cv[:, None, :]
        sr[:, :, a:b] = np.where(q == 0.0, 0.0, -pi[:, :, a:b] / q)
        si[:, :, a:b] = np.where(q == 0.0, 0.0, pr[:, :, a:b] / q)
        q = w[None, :, None] * Lv[:, None, :]
        sr[:, :, b:] = -pi[:, :, b:] * q
        si[:, :, b:] = pr[:, :, b:] * q
        hr, hi = np.zeros((ni, nf)), np.zeros((ni, nf))
        if out_p >= 0:
            hr, hi = out_v[:, :, out_p].real.copy(), out_v[:, :, out_p].imag.copy()
        if out_n >= 0:
            hr, hi = hr - out_v[:, :, out_n].real, hi - out_v[:, :, out_n].imag
        d = hr * hr + hi * hi
        hr3, hi3, d3 = hr[:, :, None], hi[:, :, None], d[:, :, None]
        m = (sr * hr3 + si * hi3) / d3
        phi = (si * hr3 - sr * hi3) / d3
        t = tol[None, None, :]
        tm, tp = t * m, t * phi
        spec = np.zeros((ni, nf, abi.SENS_SPEC))
        spec[:, :, 0], spec[:, :, 1] = hr, hi
        spec[:, :, 2] = _lane_sums(t * np.abs(m))
        spec[:, :, 3] = _lane_sums(tm * tm)
        spec[:, :, 4] = _lane_sums(t * np.abs(phi))
        spec[:, :, 5] = _lane_sums(tp * tp)
        peak = np.zeros((ni, nE, abi.SENS_PEAK))
        for col, val in ((0, m), (2, phi)):
            best = val[:, k0, :].copy()
            at = np.full((ni, nE), float(k0))
            for k in range(k0 + 1, k1 + 1):
                take = np.abs(val[:, k, :]) > np.abs(best)
                best = np.where(take, val[:, k, :], best)
                at = np.where(take, float(k), at)
            peak[:, :, col], peak[:, :, col + 1] = best, at
    return spec, peak, np.stack([m, phi], axis=3)


def _elements(ckt: ParsedCircuit) -> List[Tuple[str, str, float]]:
    """(name, kind, value) in the order of out_i's columns: R, then C, then L."""
    return [(r.name, "R", float(r.R)) for r in ckt.R] + [(c.name, "C", float(c.C)) for c in ckt.C] + [(l.name, "L", float(l.L)) for l in ckt.L]


def _tolerances(elements: List[Tuple[str, str, float]], tol) -> np.ndarray:
    def one(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"simulateSens: the tolerance of {what} must be a finite number >= 0, got {v!r}")
        return float(v)

    if tol is None:
        return np.ones(len(elements))
    if not isinstance(tol, dict):
        return np.full(len(elements), one(tol, "every element"))
    names = {n.upper() for n, _, _ in elements}
    by_name, by_kind = {}, {}
    for key, v in tol.items():
        k = str(key).upper()
        if k in names:
            by_name[k] = one(v, key)
        elif k in ("R", "C", "L"):
            by_kind[k] = one(v, f"kind {key}")
        else:
            raise ValueError(f"simulateSens: tol names {key!r}, which is neither an R, C or L of the circuit nor a kind key")
    return np.array([by_name.get(n.upper(), by_kind.get(kind, 0.0)) for n, kind, _ in elements], dtype=np.float64)


class _Plan:
    """A circuit's request resolved: the output pair, the recorded nodes, the elements and their tolerances, the window."""

    def __init__(self, ckt: ParsedCircuit, output: str, tol, freqs: np.ndarray, f_from, f_to, full: bool):
        if not len(freqs):
            raise ValueError("simulateSens: the sweep has no frequencies")
        if not str(output).strip().lower().startswith("v("):
            raise ValueError(f"simulateSens: output must be v(node) or v(node,node), got {output!r}")
        _, a, b = _parse_signal(ckt, str(output), [])
        if a == b:
            raise ValueError(f"simulateSens: {output!r}: the output pair names one node twice")
        self.elements = _elements(ckt)
        if not self.elements:
            raise ValueError("simulateSens: the circuit has no R, C or L, so there is nothing to be sensitive to")
        seen = set()
        for n, _, _ in self.elements:
            if n.upper() in seen:
                raise ValueError(f"simulateSens: two elements share the name {n!r}")
            seen.add(n.upper())
        self.tol = _tolerances(self.elements, tol)
        self.node_p, self.node_n = a, b
        self.out_nodes = sorted({n for n in (a, b) if n != 0})
        col = {n: k for k, n in enumerate(self.out_nodes)}
        self.k0, self.k1 = freq_window(freqs, f_from, f_to, "sens window")
        self.freqs = freqs
        self.full = bool(full)
        self.req = abi.ac_sens_req(col[a], col[b] if b else -1, len(ckt.R), len(ckt.C), len(ckt.L), self.k0, self.k1)
        self.key = (a, b, self.k0, self.k1, self.tol.tobytes(), self.full)

    def flatten(self, ckt: ParsedCircuit) -> abi.FlatCircuit:
        flat = abi.flatten(ckt)
        flat.out_nodes = np.ascontiguousarray(self.out_nodes, dtype=np.int32)
        return flat

    def result_bytes(self, n_freq: int) -> int:
        nE = len(self.elements)
        return n_freq * abi.SENS_SPEC * 8 + nE * abi.SENS_PEAK * 8 + (n_freq * nE * 16 if self.full else 0)

    def result(self, spec: np.ndarray, peak: np.ndarray, full: Optional[np.ndarray]) -> dict:
        """spec [n_freq][6], peak [nE][4], full [n_freq][nE][2] or None of one instance -> the result dict (module text)."""
        with np.errstate(all="ignore"):
            out = {"freqs": self.freqs.tolist(), "h": (spec[:, 0] + 1j * spec[:, 1]).tolist(),
                   "mag_wc": spec[:, 2].tolist(), "mag_sigma": np.sqrt(spec[:, 3]).tolist(),
                   "mag_wc_db": (20.0 * np.log10(1.0 + spec[:, 2])).tolist(),
                   "phase_wc_deg": np.degrees(spec[:, 4]).tolist(), "phase_sigma_deg": np.degrees(np.sqrt(spec[:, 5])).tolist(),
                   "band": (float(self.freqs[self.k0]), float(self.freqs[self.k1]))}
        rows = []
        for e, (name, kind, value) in enumerate(self.elements):
            m, km, ph, kp = (float(v) for v in peak[e])
            rows.append((name, {"kind": kind, "value": value, "tol": float(self.tol[e]), "mag_peak": m, "f_mag_peak": float(self.freqs[int(km)]),
                                "phase_peak_deg": math.degrees(ph), "f_phase_peak": float(self.freqs[int(kp)])}))

        def rank(row):
            w = abs(row[1]["mag_peak"]) * row[1]["tol"]
            return -w if w == w else -math.inf  # (a NaN ranks first: it is what the reader has to see)
        out["elements"] = dict(sorted(rows, key=rank))
        if full is not None:
            out["mag_sens"] = {n: full[:, e, 0].tolist() for e, (n, _, _) in enumerate(self.elements)}
            out["phase_sens_deg"] = {n: np.degrees(full[:, e, 1]).tolist() for e, (n, _, _) in enumerate(self.elements)}
        return out


def simulateSens(ckt: ParsedCircuit, output: str, tol=None, freqs=None, f_from: Optional[float] = None, f_to: Optional[float] = None, full: bool = False, *,
                 exact_order: bool = False, device: int = 0, backend=None) -> Optional[dict]:
    """Sensitivity analysis of `ckt` at `output` (module text).  None without a .ac card and without freqs; the errors of
    simulateAC, raised when either sweep fails at ANY frequency."""
    out = simulateSensBatch([ckt], output, tol, freqs, f_from, f_to, full, exact_order=exact_order, device=device, backend=backend)[0]
    if isinstance(out, Exception):
        raise out
    return out


def simulateSensBatch(ckts: Sequence[ParsedCircuit], output: str, tol=None, freqs=None, f_from: Optional[float] = None, f_to: Optional[float] = None,
                      full: bool = False, *, exact_order: bool = False, device: int = 0, max_instances: int = 4096, max_result_bytes: int = 1 << 30,
                      backend=None) -> List[Optional[object]]:
    """simulateSens for many circuits in as few launches as simulateACBatch would make: circuits that share topology, output
    pair, tolerances, window and frequency list are the instances of one handle, each with its own element values and source
    phasors.  Slot i is simulateSens(ckts[i], ...)'s dict, None without frequencies, or — returned, not raised — the error its
    sweeps end in.  backend: a test backend with run_ac_sens(flat, freqs, vph, node_p, node_n, req, tol, full)."""
    if exact_order:
        raise ValueError("simulateSens: the reference-order engine has no current injection (exact_order=True)")
    be = batch_backend(backend, False, device, "simulateSensBatch")
    if not hasattr(be, "run_ac_sens"):
        raise TypeError("simulateSens: the backend has no run_ac_sens (an injected sweep is not something simulateAC's backends do)")
    out: List[Optional[object]] = [None] * len(ckts)
    plans: Dict[int, _Plan] = {}

    def plan_of(c: ParsedCircuit) -> _Plan:
        if id(c) not in plans:
            plans[id(c)] = _Plan(c, output, tol, _freqs_of(c, freqs), f_from, f_to, full)
        return plans[id(c)]

    for c in ckts:  # (names, tolerances and windows are judged for every circuit before anything runs)
        if _freqs_of(c, freqs) is not None:
            plan_of(c)
    launches = ac_group_launches(ckts, out, max_instances, max_result_bytes, lambda c: plan_of(c).flatten(c),
                                 lambda flat, nf: nf * abi.SENS_SPEC * 8 + (flat.nR + flat.nC + flat.nL) * (abi.SENS_PEAK * 8 + (nf * 16 if full else 0)),
                                 lambda c, f: plan_of(c).key,
                                 freqs_override=None if freqs is None else np.asarray(freqs, dtype=np.float64).reshape(-1).tolist())
    for idx, fr in launches:
        plan = plan_of(ckts[idx[0]])
        flat, vph = stacked(ckts, idx, lambda c: plan_of(c).flatten(c))
        res = be.run_ac_sens(flat, fr, vph, plan.node_p, plan.node_n, plan.req, plan.tol, plan.full)
        ist = launch_status(res, len(idx), "simulateSensBatch")
        n_bad = int(np.count_nonzero(ist))
        for j, i in enumerate(idx):
            if int(ist[j]) != 0:
                out[i] = slot_error(int(ist[j]), res.get("detail", "") if n_bad == 1 else "")
            else:
                out[i] = plan_of(ckts[i]).result(res["spec"][j], res["peak"][j], res["full"][j] if plan.full else None)
    return out
