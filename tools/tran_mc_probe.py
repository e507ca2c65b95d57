#!/usr/bin/env python3
"""Monte Carlo of transient runs probe, JSON lines: on --inst samples of --circuit (boost_probe at --points points, or
diode_chain(--n) at --points points), one handle that records the measured nodes alone,
  plain_ms / mc_tran_ms    the transient of Handle.run_reduced and that of Handle.run_mc (spicey_last_kernel_ms: the same kernels, the
                           second bound to the drawn values), alternating --reps times in one process: every run's kernel time,
                           medians and spreads (max - min)
  draw_ms / reduce_ms      the draw's and the scalars-plus-reduction's event times (spicey_last_tran_mc_draw_ms, spicey_last_tran_mc_ms)
  bytes_back / bytes_rows / bytes_waveforms   what run_mc copies back against the passes' rows and against out_v + out_i
and, with --host-inst > 0, the wall time of measureMonteCarlo against the host route — measureTRANBatch of the mc_values variants
and np.sort on the host — at --host-inst samples, alternating --host-reps times.  --check compares run_mc with the numpy scalars and
reduction over the run_reduced rows of a second handle created from the numpy draw's values, bit for bit.  --trace-only runs one
run_mc and nothing else: the run to put under a kernel trace, whose per-kernel times split reduce_ms."""
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
from spicey_amd.lib import Handle  # noqa: E402
from spicey_amd.mc import icdf_table, mc_gains, mc_values  # noqa: E402
from spicey_amd.measure import _Plan, efficiency, measureTRANBatch, power, stats, when  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402

PROBS = (0.01, 0.5, 0.99)


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
        return text, measures, {"L": 0.05, "C": 0.10}
    text = synth.diode_chain(a.n, seed=2, tran=f".tran 1e-6 {1e-6 * (a.points - 1.5):.12g}")
    measures = {"end": stats(f"v(n{a.n})"), "mid": stats(f"v(n{a.n // 2})"), "up": when(f"v(n{a.n // 2})", 0.3)}
    return text, measures, {"R": 0.01, "C": 0.05}


def case(a, ni):
    text, measures, tol = circuit(a)
    ckt = parseNetlist(text)
    tr = ckt.analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    plan = _Plan(ckt, measures, dt, steps)
    names, sc, root = tm.compile_plan(plan, dt)
    flat = plan.flatten(ckt).replicate(ni)
    src = abi.source_table(ckt, dt, steps)
    _, t, icdf, log2K = tm._resolve(ckt, tol, "gauss", 3)
    req = abi.tran_mc_req(log2K, True, a.seed)
    h = Handle(flat)
    if a.trace_only:
        res = h.run_mc(steps, dt, src, req, t, icdf, sc, None, None, PROBS, plan.reqs, plan.treqs, plan.preqs)
        assert res["status"] == 0, res["detail"]
        h.close()
        print(json.dumps(dict(case="trace_only", circuit=a.circuit, inst=ni, points=steps + 1, reduce_ms=res["mc_ms"], draw_ms=res["draw_ms"])), flush=True)
        return
    plain, mc, draw, red = [], [], [], []
    res = None
    for _ in range(a.reps):  # (alternating: plain, mc; both from the descriptor's state)
        h.reset_state()
        p = h.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs, want_iters=False)
        assert p["status"] == 0, p["detail"]
        plain.append(p["kernel_ms"])
        h.reset_state()
        res = h.run_mc(steps, dt, src, req, t, icdf, sc, None, None, PROBS, plan.reqs, plan.treqs, plan.preqs, want_x=True)
        assert res["status"] == 0, res["detail"]
        mc.append(res["kernel_ms"])
        draw.append(res["draw_ms"])
        red.append(res["mc_ms"])
    h.reset_state()
    t0 = time.perf_counter()
    h.run_mc(steps, dt, src, req, t, icdf, sc, None, None, PROBS, plan.reqs, plan.treqs, plan.preqs)
    wall = (time.perf_counter() - t0) * 1e3
    info = h.info()
    h.close()
    n_rows = len(plan.reqs) * 8 + len(plan.treqs) * 8 + len(plan.preqs) * abi.POWER_ROW
    rec = dict(case="tran_mc", circuit=a.circuit, inst=ni, points=steps + 1, scalars=len(names), interpreter=info["interpreter"], inst_per_wg=info["inst_per_wg"],
               plain_ms=spread(plain), mc_tran_ms=spread(mc), mc_over_plain=float(np.median(mc) / np.median(plain)), draw_ms=spread(draw), reduce_ms=spread(red),
               mc_wall_ms=wall, bytes_back=int(res["stat"].nbytes + res["sample"].nbytes), bytes_x=int(res["x"].nbytes), bytes_rows=int(ni * n_rows * 8),
               bytes_waveforms=int(ni * (steps + 1) * (flat.n_out + (flat.n_cur if plan.need_i else 0)) * 8), n_nan=int(res["stat"][:, 0].sum() - res["stat"][:, 1].sum()))
    if a.check:
        g = mc_gains(ni, t, icdf, log2K, a.seed, True)
        drawn = flat.replicate(ni)
        drawn.R_val = np.ascontiguousarray(flat.R_val * g[:, :flat.nR])
        drawn.C_val = np.ascontiguousarray(flat.C_val * g[:, flat.nR:flat.nR + flat.nC])
        drawn.L_val = np.ascontiguousarray(flat.L_val * g[:, flat.nR + flat.nC:])
        h2 = Handle(drawn)
        d = h2.run_reduced(steps, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs, want_iters=False)
        h2.close()
        x = tm.eval_reference_scalars(sc, (d["meas"] if len(plan.reqs) else None, d["timing"] if len(plan.treqs) else None, d["power"] if len(plan.preqs) else None))
        rs, rf = tm.reduce_reference_tran_mc(x, None, None, None, PROBS)
        eq = lambda u, v: bool(((u.view(np.int64) == v.view(np.int64)) | (np.isnan(u) & np.isnan(v))).all())  # noqa: E731
        rec["same_bits"] = eq(rf, res["stat"]) and eq(x, res["x"]) and bool((rs == res["sample"]).all())
    print(json.dumps(rec), flush=True)


def host_route(a):
    """measureMonteCarlo against measureTRANBatch of the mc_values variants with np.sort on the host."""
    text, measures, tol = circuit(a)
    ckt = parseNetlist(text)
    n = a.host_inst
    host, dev, worst = [], [], 0.0
    for _ in range(a.host_reps):  # (alternating)
        t0 = time.perf_counter()
        variants = []
        for s in range(n):
            c = parseNetlist(text)
            vals = mc_values(c, tol, a.seed, s)
            for e in c.R:
                e.R = vals[e.name]
            for e in c.C:
                e.C = vals[e.name]
            for e in c.L:
                e.L = vals[e.name]
            variants.append(c)
        out = measureTRANBatch(variants, measures, diagnostics=False)
        fields = [(m, f) for m, d in out[0].items() for f, v in d.items() if isinstance(v, (int, float)) or v is None]
        x = np.array([[np.nan if o[m][f] is None else float(o[m][f]) for m, f in fields] for o in out])
        srt = np.sort(x, axis=0)
        host.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        r = tm.measureMonteCarlo(ckt, measures, tol=tol, n=n, seed=a.seed, quantiles=PROBS)
        dev.append(time.perf_counter() - t0)
        for j, (m, f) in enumerate(fields):
            s = r["scalars"].get(f"{m}.{f}")
            if s is None or s["n_nan"] or s["quantiles"][0.5] is None:
                continue
            pos = 0.5 * (n - 1)
            k = int(pos)
            ref = srt[k, j] + (pos - k) * (srt[min(k + 1, n - 1), j] - srt[k, j])
            worst = max(worst, abs(s["quantiles"][0.5] - ref) / max(abs(ref), 1e-300))
    print(json.dumps(dict(case="host_route", circuit=a.circuit, inst=n, points=a.points, host_wall_s=spread(host), mc_wall_s=spread(dev),
                          host_over_mc=float(np.median(host) / np.median(dev)), worst_relative_difference_of_the_medians=worst)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit", choices=("boost_probe", "diode_chain"), default="boost_probe")
    ap.add_argument("--n", type=int, default=1000, help="nodes of the diode chain")
    ap.add_argument("--points", type=int, default=10001)
    ap.add_argument("--inst", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--check", type=int, default=1)
    ap.add_argument("--trace-only", type=int, default=0)
    ap.add_argument("--host-inst", type=int, default=256)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    for ni in a.inst:
        case(a, ni)
    if a.host_inst > 0 and not a.trace_only:
        host_route(a)


if __name__ == "__main__":
    main()
