"""simulateACBatch(): many circuits' AC sweeps in as few launches as their topologies allow.

simulateAC runs one circuit per launch.  Here circuits that share node count, topology, recorded nodes and the bit pattern
of the frequency list become the instances of ONE handle, each with its own element values and source phasors
(spicey_ac_run, include/spicey_hip.h, solves every (instance, frequency) pair in one launch) — a tolerance or corner sweep
of a filter is one launch instead of one per variant.

Slot i of the result is what simulateAC(ckts[i]) returns (same keys, key order, shared-name current arrays); a circuit
without .ac gives None; an error the reference would throw — SingularComplexMatrixError, ZeroDivisionError("Complex divide
by ~0"), ValueError("R ... must be > 0") — is returned in the circuit's slot instead of raised while the others finish
(spicey_ac_last_inst_status tells the instances of a launch apart).  The resistor check of simulateAC runs per circuit on
the host before the launch, and a circuit that fails it takes no part in it.  An inductor's "Complex divide by ~0" is left
to the engines in both modes: each flags the (instance, frequency) slot where the reference's stamp throws, and an
instance's error is that of its LOWEST failing frequency index — the frequency at which the reference stops — where
simulateAC's default mode raises the inductor's error before any solve.  Exact mode gives simulateAC(c,
exact_order=True)'s bits; the default mode meets the oracle's bar (|z - z_ref| <= 1e-9 |z_ref| + 1e-12) but is not promised
to equal a solo run bit for bit (the sweep kernel depends on the batch size).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import abi
from .ac import (ERR_COMPLEX_DIV, SingularComplexMatrixError, _check_resistors,
                 ac_result, buildFrequencyArray, source_phasors)
from .netlist import ParsedCircuit


def slot_error(code: int, detail: str = "") -> Exception:
    """The exception simulateAC raises for a status code."""
    if code == abi.ERR_SINGULAR:
        return SingularComplexMatrixError(detail)
    if code == ERR_COMPLEX_DIV:
        return ZeroDivisionError("Complex divide by ~0")
    return RuntimeError(detail or f"spicey native error {code}")


def ac_group_launches(ckts: Sequence[ParsedCircuit], out: list, max_instances: int, max_result_bytes: int,
                      flatten: Callable[[ParsedCircuit], abi.FlatCircuit], inst_bytes: Callable[[abi.FlatCircuit, int], int],
                      extra: Optional[Callable[[ParsedCircuit, np.ndarray], object]] = None, freqs_override=None) -> List[tuple]:
    """The launches of a batched AC call as (indices into ckts, freqs): one group per (node count, topology, recorded nodes,
    frequency list bits[, extra(ckt, freqs)]), groups in the order they first appear, instances in input order, groups split
    so that a launch has at most max_instances instances and inst_bytes(flat, n_freq) * instances <= max_result_bytes.
    Circuits without .ac take part in none; neither do those the resistor check refuses — their exception goes to out[i].
    freqs_override: a frequency list every circuit is swept over instead of its card's (a card is then not needed)."""
    if max_instances < 1:
        raise ValueError("max_instances must be >= 1")
    groups: Dict[tuple, List[int]] = {}
    meta: Dict[tuple, tuple] = {}
    for i, c in enumerate(ckts):
        ac = c.analyses.get("ac")
        if not ac and freqs_override is None:
            continue
        freqs = buildFrequencyArray(ac["mode"], ac["N"], ac["f1"], ac["f2"]) if freqs_override is None else list(freqs_override)
        try:
            _check_resistors(c, freqs)  # (the engines raise the inductors' divide errors themselves, slot by slot)
        except ValueError as e:
            out[i] = e
            continue
        f = np.asarray(freqs, dtype=np.float64)
        flat = flatten(c)
        topo = tuple(getattr(flat, k).tobytes() for k in abi.FlatCircuit.TOPO)
        nodes = None if flat.out_nodes is None else tuple(int(n) for n in flat.out_nodes)
        key = (flat.n_nodes, topo, nodes, f.tobytes())
        if extra is not None:
            key = key + (extra(c, f),)
        groups.setdefault(key, []).append(i)
        meta.setdefault(key, (f, max(1, inst_bytes(flat, len(f)))))
    launches = []
    for key, idx in groups.items():
        f, per = meta[key]
        cap = max(1, min(max_instances, max_result_bytes // per))
        launches += [(idx[a:a + cap], f) for a in range(0, len(idx), cap)]
    return launches


def stacked(ckts: Sequence[ParsedCircuit], idx: List[int], flatten) -> tuple:
    """(FlatCircuit of the launch, phasors [n_inst][nV])."""
    flats = [flatten(ckts[i]) for i in idx]
    flat = abi.stack_instances(flats) if len(flats) > 1 else flats[0]
    vph = np.stack([source_phasors(ckts[i]) for i in idx]) if idx else np.zeros((0, 0), np.complex128)
    return flat, vph


def launch_status(res: dict, n_inst: int, who: str) -> np.ndarray:
    """Per-instance status of a launch's result; raises for what is no circuit's own error."""
    rc = res["status"]
    if rc not in (abi.OK, abi.ERR_SINGULAR, ERR_COMPLEX_DIV):
        raise RuntimeError(res.get("detail") or f"spicey native error {rc}")
    ist = res.get("inst_status")
    if ist is None:
        if rc != abi.OK and n_inst > 1:
            raise RuntimeError(f"{who}: the backend reported a failing sweep without per-instance status")
        ist = np.full(n_inst, rc, np.int32)
    return np.asarray(ist)


def batch_backend(backend, exact_order: bool, device: int, who: str):
    if exact_order and backend is not None:
        raise ValueError(f"{who}: pass either backend= or exact_order=True, not both")
    if backend is not None:
        return backend
    from .lib import HipAcExactBackend, HipBackend

    return HipAcExactBackend(device=device) if exact_order else HipBackend(device=device)


def _result_bytes(flat: abi.FlatCircuit, n_freq: int) -> int:
    return n_freq * (flat.n_out + flat.nR + flat.nC + flat.nL + flat.nV) * 16


def simulateACBatch(ckts: Sequence[ParsedCircuit], *, exact_order: bool = False, device: int = 0, max_instances: int = 4096,
                    max_result_bytes: int = 1 << 30, backend=None) -> List[Optional[object]]:
    """AC sweep of every circuit in `ckts`; see the module text.  backend: a test backend whose run_ac(flat, freqs, vph,
    want_currents) accepts phasors [n_inst][nV] and reports `inst_status`."""
    be = batch_backend(backend, exact_order, device, "simulateACBatch")
    out: List[Optional[object]] = [None] * len(ckts)
    for idx, freqs in ac_group_launches(ckts, out, max_instances, max_result_bytes, abi.flatten, _result_bytes):
        flat, vph = stacked(ckts, idx, abi.flatten)
        res = be.run_ac(flat, freqs, vph, want_currents=True)
        ist = launch_status(res, len(idx), "simulateACBatch")
        n_bad = int(np.count_nonzero(ist))
        for j, i in enumerate(idx):
            if int(ist[j]) != 0:
                out[i] = slot_error(int(ist[j]), res.get("detail", "") if n_bad == 1 else "")
            else:
                out[i] = ac_result(ckts[i], freqs.tolist(), res["out_v"][j], res["out_i"][j])
    return out
