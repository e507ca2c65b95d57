#!/usr/bin/env python3
"""Sensitivities and corners of transient measurements probe, JSON lines: on the one-at-a-time design of --circuit (boost_probe at
--points points, or diode_chain(--n) at --points points; --active > 0 keeps only the first --active toleranced elements), one handle
of 1 + 2 nA instances that records the measured nodes alone,
  plain_ms / sens_tran_ms   the transient of Handle.run_reduced and that of Handle.run_sens (spicey_last_kernel_ms: the same kernels,
                            the second bound to the designed values), alternating --reps times in one process: every run's kernel
                            time, medians and spreads (max - min)
  design_ms / reduce_ms     the design's and the scalars-plus-reduction's event times (spicey_last_tran_sens_design_ms,
                            spicey_last_tran_sens_ms)
  bytes_back / bytes_rows / bytes_waveforms   what run_sens copies back against the passes' rows and against out_v + out_i
and, with --host-reps > 0, the wall time of measureWorstCase against the host route — measureTRANBatch of the design_circuit
variants twice (the one-at-a-time design, then the corners), the differences in numpy — alternating --host-reps times.  --check
compares run_sens with the numpy scalars and reduction over the run_reduced rows of a second handle created from the numpy
design's values, bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import golden_netlist, load_golden  # noqa: E402
from spicey_amd import abi, synth  # noqa: E402
from spicey_amd import tran_mc as tm  # noqa: E402
from spicey_amd import tran_sens as ts  # noqa: E402
from spicey_amd.lib import Handle  # noqa: E402
from spicey_amd.measure import _Plan, efficiency, measureTRANBatch, power, stats, when  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402


def spread(xs):
    return {"runs": [round(x, 4) for x in xs], "median": float(np.median(xs)), "spread": float(max(xs) - min(xs))}


def circuit(a):
    """(netlist text, measures, tol) of the probe's circuit at a.points points."""
    if a.circuit == "boost_probe":
        base = golden_netlist(load_golden("boost_probe"))
        text = "\n".join(f".tran {0.1 / (a.points - 1):.12g} 0.1 uic" if ln.lower().startswith(".tran") else ln for ln in base.splitlines()
                         if not ln.upper().startswith(".PRINT")) + "\n"
        measures = {"ripple": stats("v(n3)", t_from=0.08), "rise": when("v(n3)", 5.5), "pl": power("RR1"),
                    "eff": efficiency(power("RR1"), power("Vsimulation_voltage_source_0"))}
        tol = {"R": 0.01, "L": 0.05, "C": 0.10}
    else:
        text = synth.diode_chain(a.n, seed=2, tran=f".tran 1e-6 {1e-6 * (a.points - 1.5):.12g}")
        measures = {"end": stats(f"v(n{a.n})"), "mid": stats(f"v(n{a.n // 2})"), "up": when(f"v(n{a.n // 2})", 0.3)}
        tol = {"R": 0.01, "C": 0.05}
    if a.active > 0:  # only the first a.active toleranced elements, by name
        ckt = parseNetlist(text)
        elements, t, act, _ = ts._resolve_design(ckt, tol, 1e-3)
        tol = {elements[int(e)][0]: float(t[int(e)]) for e in act[:a.active]}
    return text, measures, tol


def case(a):
    text, measures, tol = circuit(a)
    ckt = parseNetlist(text)
    tr = ckt.analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    plan = _Plan(ckt, measures, dt, steps)
    names, sc, root = tm.compile_plan(plan, dt)
    elements, t, act, h_step = ts._resolve_design(ckt, tol, a.rel_step)
    nA = len(act)
    ni = 1 + 2 * nA
    flat = plan.flatten(ckt).replicate(ni)
    src = abi.source_table(ckt, dt, steps)
    req = abi.tran_sens_req(abi.TS_ONE_AT_A_TIME, nA)
    h = Handle(flat)
    plain, sens, design, red = [], [], [], []
    res = None
    for _ in range(a.reps):  # (alternating: plain, sens; both from the descriptor's state)
        h.reset_state()
        p = h.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs, want_iters=False)
        assert p["status"] == 0, p["detail"]
        plain.append(p["kernel_ms"])
        h.reset_state()
        res = h.run_sens(steps, dt, src, req, act, h_step, t, sc, plan.reqs, plan.treqs, plan.preqs, want_x=True)
        assert res["status"] == 0, res["detail"]
        sens.append(res["kernel_ms"])
        design.append(res["design_ms"])
        red.append(res["sens_ms"])
    info = h.info()
    h.close()
    n_rows = len(plan.reqs) * 8 + len(plan.treqs) * 8 + len(plan.preqs) * abi.POWER_ROW
    rec = dict(case="tran_sens", circuit=a.circuit, nA=nA, inst=ni, points=steps + 1, scalars=len(names), interpreter=info["interpreter"], inst_per_wg=info["inst_per_wg"],
               plain_ms=spread(plain), sens_tran_ms=spread(sens), sens_over_plain=float(np.median(sens) / np.median(plain)), design_ms=spread(design),
               reduce_ms=spread(red), bytes_back=int(res["sens"].nbytes + res["sign"].nbytes + res["bound"].nbytes), bytes_x=int(res["x"].nbytes),
               bytes_rows=int(ni * n_rows * 8), bytes_waveforms=int(ni * (steps + 1) * (flat.n_out + (flat.n_cur if plan.need_i else 0)) * 8),
               n_nan=int(nA * len(names) - res["bound"][:, 3].sum()), n_interior=int(res["bound"][:, 6].sum()))
    if a.check:
        designed = flat.replicate(ni)
        designed.R_val, designed.C_val, designed.L_val = (np.ascontiguousarray(v) for v in ts.design_values(flat.R_val, flat.C_val, flat.L_val, act, h_step))
        h2 = Handle(designed)
        d = h2.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs, want_iters=False)
        h2.close()
        x = tm.eval_reference_scalars(sc, (d["meas"] if len(plan.reqs) else None, d["timing"] if len(plan.treqs) else None, d["power"] if len(plan.preqs) else None))
        rsens, rsign, rbound = ts.reduce_reference_tran_sens(x, None, h_step, t[act])
        eq = lambda u, v: bool(((u.view(np.int64) == v.view(np.int64)) | (np.isnan(u) & np.isnan(v))).all())  # noqa: E731
        rec["same_bits"] = eq(x, res["x"]) and eq(rsens, res["sens"]) and eq(rbound, res["bound"]) and bool((rsign == res["sign"]).all())
    print(json.dumps(rec), flush=True)


def _variants(text, ckt, tol, n, rel_step, levels=None):
    out = []
    for s in range(n):
        c = parseNetlist(text)
        vals = ts.design_circuit(ckt, tol, s, rel_step, levels)
        for e in c.R:
            e.R = vals[e.name]
        for e in c.C:
            e.C = vals[e.name]
        for e in c.L:
            e.L = vals[e.name]
        out.append(c)
    return out


def _fields(out):
    fields = [(m, f) for m, d in out[0].items() for f, v in d.items() if isinstance(v, (int, float)) or v is None]
    return fields, np.array([[np.nan if o[m][f] is None else float(o[m][f]) for m, f in fields] for o in out])


def host_route(a):
    """measureWorstCase against measureTRANBatch of the design_circuit variants twice, with the differences in numpy."""
    text, measures, tol = circuit(a)
    ckt = parseNetlist(text)
    elements, t, act, h_step = ts._resolve_design(ckt, tol, a.rel_step)
    nA = len(act)
    host, dev, worst, n_corners = [], [], 0.0, 0
    for _ in range(a.host_reps):  # (alternating)
        t0 = time.perf_counter()
        fields, x = _fields(measureTRANBatch(_variants(text, ckt, tol, 1 + 2 * nA, a.rel_step), measures, diagnostics=False))
        with np.errstate(all="ignore"):
            d = (x[1::2] - x[2::2]) / (2.0 * h_step[:, None])
        sign = np.where(np.isnan(d), 0, np.sign(d)).astype(np.int8).T
        lvl, idx = ts.corner_rows(sign, act, len(elements))
        _, xc = _fields(measureTRANBatch(_variants(text, ckt, tol, len(lvl), a.rel_step, lvl), measures, diagnostics=False))
        host.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        r = ts.measureWorstCase(ckt, measures, tol=tol, rel_step=a.rel_step)
        dev.append(time.perf_counter() - t0)
        n_corners = r["n_corners"]
        for j, (m, f) in enumerate(fields):
            s = r["scalars"].get(f"{m}.{f}")
            if s is None or s["corner_high"] is None or np.isnan(xc[idx[j, 0], j]) or len(lvl) != len(r["corner_levels"]):
                continue
            worst = max(worst, abs(s["corner_high"] - xc[idx[j, 0], j]) / max(abs(xc[idx[j, 0], j]), 1e-300))
    print(json.dumps(dict(case="host_route", circuit=a.circuit, nA=nA, inst=1 + 2 * nA, corners=n_corners, points=a.points, host_wall_s=spread(host),
                          worst_case_wall_s=spread(dev), host_over_device=float(np.median(host) / np.median(dev)),
                          worst_relative_difference_of_the_high_corners=worst)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit", choices=("boost_probe", "diode_chain"), default="boost_probe")
    ap.add_argument("--n", type=int, default=1000, help="nodes of the diode chain")
    ap.add_argument("--points", type=int, default=10001)
    ap.add_argument("--active", type=int, default=0, help="keep only the first ACTIVE toleranced elements (0: all)")
    ap.add_argument("--rel-step", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    if a.reps > 0:
        case(a)
    if a.host_reps > 0:
        host_route(a)


if __name__ == "__main__":
    main()
