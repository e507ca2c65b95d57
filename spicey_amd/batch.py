"""simulateTRANBatch(): many circuits' transients in as few launches as their topologies allow.

simulateTRAN runs one circuit per launch.  Here circuits that share a topology, recorded nodes, dt and step count become the
instances of ONE handle, each driven by its own source table (spicey_run_src, include/spicey_hip.h) — a sweep of element
values, supply corners, input amplitudes or PWL test vectors is one launch instead of one per variant.

Slot i of the result is what simulateTRAN(ckts[i], exact_order=...) returns (same keys, key order, times, .PRINT
filtering, shared-name current arrays, `iterations`, `skipRisk`) and the circuit's state is written back the same way; a
circuit without .tran gives None and one whose run is singular gives its SingularMatrixError, returned instead of raised,
with its state left as it was.  Exact mode gives simulateTRAN(c, exact_order=True)'s bits; the default mode meets the
oracle's bar with the same iteration counts, but is not promised to equal a solo run bit for bit (K, workgroup geometry
and the tridiagonal top depend on the batch size).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from . import abi
from .netlist import ParsedCircuit, js_object_key_order
from .simulate import SingularMatrixError


def _group_key(ckt: ParsedCircuit, flat: abi.FlatCircuit, dt: float, steps: int) -> tuple:
    # (abi.stack_instances compares the topology arrays only; the recorded nodes must agree as well)
    topo = tuple(getattr(flat, k).tobytes() for k in abi.FlatCircuit.TOPO)
    out = None if flat.out_nodes is None else tuple(int(i) for i in flat.out_nodes)
    return (flat.n_nodes, topo, out, dt, steps)


def _probe_flatten(ckt: ParsedCircuit) -> abi.FlatCircuit:
    return abi.flatten(ckt, probe_filter=True)


def group_launches(ckts: Sequence[ParsedCircuit], max_instances: int, flatten, extra=None) -> List[List[int]]:
    """batch_launches for any flattening (`flatten(ckt)` decides the recorded nodes); `extra(ckt, dt, steps)`, if given,
    joins the group key."""
    if max_instances < 1:
        raise ValueError("max_instances must be >= 1")
    groups: Dict[tuple, List[int]] = {}
    for i, c in enumerate(ckts):
        tran = c.analyses.get("tran")
        if not tran:
            continue
        dt, steps = abi.computeEffectiveTimeStep(tran["dt"], tran["tstop"])
        key = _group_key(c, flatten(c), dt, steps)
        if extra is not None:
            key = key + (extra(c, dt, steps),)
        groups.setdefault(key, []).append(i)
    return [idx[a:a + max_instances] for idx in groups.values() for a in range(0, len(idx), max_instances)]


def batch_launches(ckts: Sequence[ParsedCircuit], max_instances: int = 4096) -> List[List[int]]:
    """The launches simulateTRANBatch makes, as lists of indices into `ckts`: one group per (node count, topology, recorded
    nodes, dt, steps), groups in the order they first appear, instances in input order, groups above `max_instances` split
    into consecutive launches.  Circuits without .tran take part in none."""
    return group_launches(ckts, max_instances, _probe_flatten)


def write_state(ckt: ParsedCircuit, state: dict, j: int) -> None:
    """simulateTRAN's state write-back (spicey_amd/simulate.py) from instance j of a batched run."""
    for k, c in enumerate(ckt.C):
        c.vPrev = float(state["C_vprev"][j, k])
    for k, l in enumerate(ckt.L):
        l.iPrev = float(state["L_iprev"][j, k])
    for k, d in enumerate([d for d in ckt.D if d.model is not None]):
        d.vdPrev = float(state["D_vdprev"][j, k])
    for k, s in enumerate([s for s in ckt.S if s.model is not None]):
        s.isOn = bool(state["S_ison"][j, k])


def _tran_result(ckt: ParsedCircuit, flat: abi.FlatCircuit, dt: float, steps: int, out_v: np.ndarray, out_i: np.ndarray,
                 iters, state: dict, j: int, skip) -> dict:
    """simulateTRAN's re-keying and state write-back (spicey_amd/simulate.py) for instance j of a batched run."""
    times = [step * dt for step in range(steps + 1)]
    times[0] = 0.0
    names = ckt.nodes.rev
    if len(ckt.probes["tran"]) > 0:
        recorded = [int(i) for i in flat.out_nodes] if flat.out_nodes is not None else []
    else:
        recorded = list(range(1, ckt.nodes.count()))
    col = {names[i]: c for c, i in enumerate(recorded)}
    node_voltages = {name: out_v[:, col[name]].tolist() for name in js_object_key_order([names[i] for i in recorded])}
    elem_names: List[str] = ([e.name for e in ckt.R] + [e.name for e in ckt.C] + [e.name for e in ckt.L]
                             + [e.name for e in ckt.V] + [e.name for e in ckt.S if e.model is not None]
                             + [e.name for e in ckt.D if e.model is not None])
    groups: Dict[str, List[int]] = {}
    for k, nm in enumerate(elem_names):
        groups.setdefault(nm, []).append(k)
    element_currents = {}
    for nm in js_object_key_order(elem_names):
        cols = groups[nm]
        element_currents[nm] = out_i[:, cols[0]].tolist() if len(cols) == 1 else out_i[:, cols].reshape(-1).tolist()
    write_state(ckt, state, j)
    return {"times": times, "nodeVoltages": node_voltages, "elementCurrents": element_currents,
            "iterations": iters[j:j + 1] if iters is not None else None, "skipRisk": skip}


def run_launch(run, ckts: Sequence[ParsedCircuit], idx: List[int], out: list, diagnostics: bool, flatten, result, who: str) -> None:
    """One group's launch, then follow-up launches for the instances a failing workgroup mate stopped (inst_status -1).
    Each round settles at least one failing instance, so this ends; with one instance per workgroup (exact mode, circuits
    with switches) no follow-up is needed.  Every round starts from the circuits' own (host) state: instances that did not
    finish were not written back.
    run(flat, steps, dt, src) -> the backend's result dict; flatten(ckt) -> FlatCircuit;
    result(i, flat_i, dt, steps, res, j, skip) -> slot i's value from instance j of `res` (it writes the state back)."""
    tran = ckts[idx[0]].analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tran["dt"], tran["tstop"])
    pending = list(idx)
    while pending:
        flats = [flatten(ckts[i]) for i in pending]
        flat = abi.stack_instances(flats) if len(flats) > 1 else flats[0]
        tabs = abi.source_tables([ckts[i] for i in pending], dt, steps)
        # (bit patterns: a table that differs only in the sign of a zero is another table)
        shared = all(np.array_equal(t.view(np.int64), tabs[0].view(np.int64)) for t in tabs[1:])
        res = run(flat, steps, dt, tabs[0] if shared else tabs)
        rc = res["status"]
        if rc not in (abi.OK, abi.ERR_SINGULAR):
            raise RuntimeError(res.get("detail", f"spicey native error {rc}"))
        ist = res.get("inst_status")
        if ist is None:
            if rc != abi.OK:
                raise RuntimeError(f"{who}: the backend reported a singular run without per-instance status")
            ist = np.zeros(len(pending), np.int32)
        # results of finished instances are there when the run succeeded, or when the backend returned them after a failure
        # (`partial`) together with their diagnostics; otherwise they run again with the stopped ones
        skip = res.get("skip_risk")
        have = rc == abi.OK or (bool(res.get("partial")) and (skip is not None or not diagnostics))
        again = []
        for j, i in enumerate(pending):
            s = int(ist[j])
            if s == 0 and have:
                sk = (int(skip[j]) if skip is not None else 0) if diagnostics else None
                out[i] = result(i, flats[j], dt, steps, res, j, sk)
            elif s == abi.ERR_SINGULAR:
                out[i] = SingularMatrixError(res.get("detail", "") if int(np.count_nonzero(ist == abi.ERR_SINGULAR)) == 1 else "")
            elif s in (0, -1):  # (0 here: finished, but its results or diagnostics did not come back)
                again.append(i)
            else:
                raise RuntimeError(res.get("detail", f"spicey native error {s} (batch slot {i})"))
        if len(again) == len(pending):  # (no instance settled: a backend that contradicts itself)
            raise RuntimeError(f"{who}: a launch settled none of its instances")
        pending = again


def _run_launch(be, ckts: Sequence[ParsedCircuit], idx: List[int], out: list, diagnostics: bool) -> None:
    """simulateTRANBatch's launches: the .PRINT nodes recorded, currents wanted, slots re-keyed like simulateTRAN's result."""
    run_launch(lambda flat, steps, dt, src: be.run(flat, steps, dt, src, want_currents=True), ckts, idx, out, diagnostics, _probe_flatten,
               lambda i, flat_i, dt, steps, res, j, sk: _tran_result(ckts[i], flat_i, dt, steps, res["out_v"][j], res["out_i"][j], res.get("iters"),
                                                                      res["state"], j, sk),
               "simulateTRANBatch")


def simulateTRANBatch(ckts: Sequence[ParsedCircuit], *, exact_order: bool = False, diagnostics: bool = True, device: int = 0,
                      max_instances: int = 4096, backend=None) -> List[Optional[object]]:
    """Transient of every circuit in `ckts`; see the module text.  diagnostics=False creates the handles without
    diagnostics — eligible for the throughput geometry, K = 4 and the hybrid workspace — and `skipRisk` is then None.
    backend: a test backend whose run(flat, steps, dt, src, want_currents) accepts [n_inst][steps+1][nV] tables and
    reports `inst_status`."""
    seen = set()
    for c in ckts:
        if id(c) in seen:
            raise ValueError("simulateTRANBatch: the same circuit object appears twice (its state would be written twice)")
        seen.add(id(c))
    if exact_order and backend is not None:
        raise ValueError("simulateTRANBatch: pass either backend= or exact_order=True, not both")
    out: List[Optional[object]] = [None] * len(ckts)
    launches = batch_launches(ckts, max_instances)
    if not launches:
        return out
    if backend is None:
        from .lib import HipBackend  # fails loudly if the extension is missing

        backend = HipBackend(device=device, diagnostics=1 if diagnostics else 0, interpreter=3 if exact_order else 0)
    for idx in launches:
        _run_launch(backend, ckts, idx, out, diagnostics)
    return out
