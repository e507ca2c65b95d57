"""simulateNoise() / simulateNoiseBatch(): thermal noise, output impedance and gain of the small-signal circuit.

The reference has no current source, so what needs something injected at the output — an output impedance, the noise at a
node — is out of simulateAC's reach.  Here ONE sweep of the AC engine runs with every source phasor at zero and a unit
current injected into the output pair (spicey_ac_run_noise, include/spicey_hip.h).  The AC matrix of R, C, L and V is
complex symmetric, so that solution is the adjoint one (DESIGN.md "Noise analysis"): with out = v(p) - v(n),

    v(p) - v(n)      is Z_out(f)
    i(V_in)          is the voltage gain V_in -> out
    i(R_k)           is the gain to out of a voltage source in series with R_k

and the output noise density is the sum over the resistors of 4kT R_k |i(R_k)|^2.  The sweep's buffers stay on the device;
a reduction pass brings back 4 doubles per frequency and one per resistor.  Capacitors and inductors are noiseless, sources
are short circuits; diodes and switches take no part, as in simulateAC.

    simulateNoise(ckt, output="v(out)" | "v(a,b)", input=None | "V1", temp=300.15, freqs=None, f_from=None, f_to=None)

freqs defaults to the .ac card's list (None is returned without either); f_from / f_to select the band the totals and
contributions are integrated over (trapezoidal rule on the listed frequencies; a band of one frequency integrates to 0).
The result:

    freqs                                   the sweep's frequencies, Hz
    onoise, onoise_rms_density              V^2/Hz and V/sqrt(Hz) at the output
    zout                                    complex output impedance
    gain, inoise                            the complex voltage gain input -> output, and onoise / |gain|^2 (None without `input`)
    total, total_rms                        onoise integrated over the band, V^2 and V
    total_in, total_in_rms                  the same referred to the input (None without `input`)
    contributions                           {resistor name: V^2 over the band}, largest first (resistors that share a
                                            name share an entry)

simulateNoiseBatch groups, splits and reports per-slot errors exactly like simulateACBatch.  reduce_reference_noise() is the
same definition in plain numpy; it is what the tests compare the device with.  The reference-order engine has no injection:
exact_order=True raises.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .ac import buildFrequencyArray
from .ac_batch import ac_group_launches, batch_backend, launch_status, slot_error, stacked
from .ac_measure import freq_window
from .measure import _parse_signal
from .netlist import ParsedCircuit

K_B = 1.380649e-23  # J/K (exact, SI 2019)
LANES = 64


def kt4_of(temp: float) -> float:
    """4 k_B T as the host forms it: (4 k_B) T, two rounded products."""
    return (4.0 * K_B) * float(temp)


def reduce_reference_noise(out_v: np.ndarray, out_i: np.ndarray, R: np.ndarray, freqs: np.ndarray, kt4: float, out_p: int, out_n: int,
                           in_col: int, k_from: int = 0, k_to: int = -1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The definition of spicey_ac_noise_device in numpy, independent of the kernels: out_v complex [n_inst][n_freq][n_v] and
    out_i complex [n_inst][n_freq][n_i] of an injected sweep (the first nR columns of out_i are the resistors), R
    [n_inst][nR] ohms -> (spec [n_inst][n_freq][4], contrib [n_inst][nR], total [n_inst][2]).  Every product, sum and quotient
    is one numpy operation, rounded on its own, in the order of noise_exec.h: per resistor p = re re + im im, c = (kt4 R) p;
    per (instance, frequency) 64 lane sums over r = l, l + 64, ... in ascending r, met by s[l] += s[l + stride] for stride =
    32 .. 1; per band acc += (0.5 (y_k + y_k+1)) (f_k+1 - f_k) in ascending k from +0.0."""
    out_v = np.asarray(out_v, dtype=np.complex128)
    out_i = np.asarray(out_i, dtype=np.complex128)
    R = np.asarray(R, dtype=np.float64)
    freqs = np.asarray(freqs, dtype=np.float64)
    ni, nf = out_i.shape[0], out_i.shape[1]
    nR = R.shape[1]
    k1 = nf - 1 if k_to == -1 else int(k_to)
    k0 = int(k_from)
    if not (0 <= k0 <= k1 < nf) or out_p == out_n or nR < 1 or nR > out_i.shape[2]:
        raise ValueError("reduce_reference_noise: bad request")
    re, im = out_i[:, :, :nR].real, out_i[:, :, :nR].imag
    with np.errstate(all="ignore"):
        p = re * re + im * im
        c = (np.float64(kt4) * R)[:, None, :] * p
        groups = (nR + LANES - 1) // LANES
        pad = np.zeros((ni, nf, groups * LANES))
        pad[:, :, :nR] = c
        pad = pad.reshape(ni, nf, groups, LANES)
        s = np.zeros((ni, nf, LANES))
        for g in range(groups):
            s = s + pad[:, :, g, :]  # (a lane past the last resistor adds +0.0: no change to a sum that is >= 0 or NaN)
        stride = LANES // 2
        while stride:
            s[:, :, :stride] = s[:, :, :stride] + s[:, :, stride:2 * stride]
            stride //= 2
        spec = np.zeros((ni, nf, abi.NOISE_SPEC))
        spec[:, :, 0] = s[:, :, 0]
        if in_col >= 0:
            g = out_i[:, :, in_col]
            spec[:, :, 1] = g.real * g.real + g.imag * g.imag
        zr, zi = np.zeros((ni, nf)), np.zeros((ni, nf))
        if out_p >= 0:
            zr, zi = out_v[:, :, out_p].real.copy(), out_v[:, :, out_p].imag.copy()
        if out_n >= 0:
            zr, zi = zr - out_v[:, :, out_n].real, zi - out_v[:, :, out_n].imag
        spec[:, :, 2], spec[:, :, 3] = zr, zi

        def band(y):  # y [n_inst][n_freq][...]
            acc = np.zeros(y[:, 0].shape)
            for k in range(k0, k1):
                acc = acc + (0.5 * (y[:, k] + y[:, k + 1])) * (freqs[k + 1] - freqs[k])
            return acc

        contrib = band(c)
        total = np.stack([band(spec[:, :, 0]), band(spec[:, :, 0] / spec[:, :, 1])], axis=1)
    return spec, contrib, total


class _Plan:
    """A circuit's request resolved: the output pair, the recorded nodes, the input source's column, the band."""

    def __init__(self, ckt: ParsedCircuit, output: str, input: Optional[str], temp: float, freqs: np.ndarray, f_from, f_to):
        if not len(freqs):
            raise ValueError("simulateNoise: the sweep has no frequencies")
        if not (isinstance(temp, (int, float)) and math.isfinite(temp) and temp >= 0):
            raise ValueError(f"simulateNoise: temp must be a finite temperature in kelvin >= 0, got {temp!r}")
        if not str(output).strip().lower().startswith("v("):
            raise ValueError(f"simulateNoise: output must be v(node) or v(node,node), got {output!r}")
        _, a, b = _parse_signal(ckt, str(output), [])
        if a == b:
            raise ValueError(f"simulateNoise: {output!r}: the output pair names one node twice")
        if not ckt.R:
            raise ValueError("simulateNoise: the circuit has no resistor, so nothing makes thermal noise")
        self.node_p, self.node_n = a, b
        self.out_nodes = sorted({n for n in (a, b) if n != 0})
        col = {n: k for k, n in enumerate(self.out_nodes)}
        self.in_col = -1
        if input is not None:
            hits = [k for k, v in enumerate(ckt.V) if v.name.upper() == str(input).upper()]
            if len(hits) != 1:
                raise ValueError(f"simulateNoise: input {input!r}: " + ("no voltage source of that name" if not hits else f"{len(hits)} sources share the name"))
            self.in_col = len(ckt.R) + len(ckt.C) + len(ckt.L) + hits[0]
        self.k0, self.k1 = freq_window(freqs, f_from, f_to, "noise band")
        self.freqs = freqs
        self.kt4 = kt4_of(temp)
        self.req = abi.ac_noise_req(col[a], col[b] if b else -1, self.in_col, self.kt4, self.k0, self.k1)
        self.key = (a, b, self.in_col, self.k0, self.k1, np.float64(self.kt4).tobytes())

    def flatten(self, ckt: ParsedCircuit) -> abi.FlatCircuit:
        flat = abi.flatten(ckt)
        flat.out_nodes = np.ascontiguousarray(self.out_nodes, dtype=np.int32)
        return flat

    def result(self, ckt: ParsedCircuit, spec: np.ndarray, contrib: np.ndarray, total: np.ndarray) -> dict:
        """spec [n_freq][4], contrib [nR], total [2] of one instance -> the result dict (module text)."""
        onoise, gain2 = spec[:, 0], spec[:, 1]
        have_in = self.in_col >= 0
        with np.errstate(all="ignore"):
            inoise = (onoise / gain2).tolist() if have_in else None
        shares: Dict[str, float] = {}
        for r, v in zip(ckt.R, contrib.tolist()):
            shares[r.name] = shares.get(r.name, 0.0) + v
        ranked = dict(sorted(shares.items(), key=lambda kv: -kv[1] if kv[1] == kv[1] else math.inf))
        t_out, t_in = float(total[0]), float(total[1])
        return {"freqs": self.freqs.tolist(), "onoise": onoise.tolist(), "onoise_rms_density": np.sqrt(onoise).tolist(),
                "zout": (spec[:, 2] + 1j * spec[:, 3]).tolist(),
                "gain": None, "inoise": inoise,
                "total": t_out, "total_rms": math.sqrt(t_out) if t_out >= 0 else math.nan,
                "total_in": t_in if have_in else None,
                "total_in_rms": (math.sqrt(t_in) if t_in >= 0 else math.nan) if have_in else None,
                "contributions": ranked, "band": (float(self.freqs[self.k0]), float(self.freqs[self.k1]))}


def _freqs_of(ckt: ParsedCircuit, freqs) -> Optional[np.ndarray]:
    if freqs is not None:
        return np.asarray(freqs, dtype=np.float64).reshape(-1)
    ac = ckt.analyses.get("ac")
    if not ac:
        return None
    return np.asarray(buildFrequencyArray(ac["mode"], ac["N"], ac["f1"], ac["f2"]), dtype=np.float64)


def simulateNoise(ckt: ParsedCircuit, output: str, input: Optional[str] = None, temp: float = 300.15, freqs=None, f_from: Optional[float] = None,
                  f_to: Optional[float] = None, *, exact_order: bool = False, device: int = 0, backend=None) -> Optional[dict]:
    """Noise analysis of `ckt` at `output` (module text).  None without a .ac card and without freqs; the errors of
    simulateAC, raised when the sweep fails at ANY frequency."""
    out = simulateNoiseBatch([ckt], output, input, temp, freqs, f_from, f_to, exact_order=exact_order, device=device, backend=backend)[0]
    if isinstance(out, Exception):
        raise out
    return out


def simulateNoiseBatch(ckts: Sequence[ParsedCircuit], output: str, input: Optional[str] = None, temp: float = 300.15, freqs=None,
                       f_from: Optional[float] = None, f_to: Optional[float] = None, *, exact_order: bool = False, device: int = 0,
                       max_instances: int = 4096, max_result_bytes: int = 1 << 30, backend=None) -> List[Optional[object]]:
    """simulateNoise for many circuits in as few launches as simulateACBatch would make: circuits that share topology, output
    pair, input source, band and frequency list are the instances of one handle, each with its own element values.  Slot i
    is simulateNoise(ckts[i], ...)'s dict, None without frequencies, or — returned, not raised — the error its sweep ends
    in.  backend: a test backend with run_ac_noise(flat, freqs, node_p, node_n, req)."""
    if exact_order:
        raise ValueError("simulateNoise: the reference-order engine has no current injection (exact_order=True)")
    be = batch_backend(backend, False, device, "simulateNoiseBatch")
    if not hasattr(be, "run_ac_noise"):
        raise TypeError("simulateNoise: the backend has no run_ac_noise (an injected sweep is not something simulateAC's backends do)")
    out: List[Optional[object]] = [None] * len(ckts)
    plans: Dict[int, _Plan] = {}

    def plan_of(c: ParsedCircuit) -> _Plan:
        if id(c) not in plans:
            plans[id(c)] = _Plan(c, output, input, temp, _freqs_of(c, freqs), f_from, f_to)
        return plans[id(c)]

    for c in ckts:  # (names and bands are judged for every circuit before anything runs)
        if _freqs_of(c, freqs) is not None:
            plan_of(c)
    launches = ac_group_launches(ckts, out, max_instances, max_result_bytes, lambda c: plan_of(c).flatten(c),
                                 lambda flat, nf: nf * abi.NOISE_SPEC * 8 + flat.nR * 8 + 16, lambda c, f: plan_of(c).key,
                                 freqs_override=None if freqs is None else np.asarray(freqs, dtype=np.float64).reshape(-1).tolist())
    for idx, fr in launches:
        plan = plan_of(ckts[idx[0]])
        flat, _ = stacked(ckts, idx, lambda c: plan_of(c).flatten(c))
        res = be.run_ac_noise(flat, fr, plan.node_p, plan.node_n, plan.req)
        ist = launch_status(res, len(idx), "simulateNoiseBatch")
        n_bad = int(np.count_nonzero(ist))
        for j, i in enumerate(idx):
            if int(ist[j]) != 0:
                out[i] = slot_error(int(ist[j]), res.get("detail", "") if n_bad == 1 else "")
            else:
                r = plan_of(ckts[i]).result(ckts[i], res["spec"][j], res["contrib"][j], res["total"][j])
                if plan.in_col >= 0 and res.get("gain") is not None:
                    r["gain"] = np.asarray(res["gain"][j]).tolist()
                out[i] = r
    return out
