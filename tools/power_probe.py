#!/usr/bin/env python3
"""Cost of the device-side product pass (spicey_power_device, Handle.run_measure_power, power() / efficiency()), one JSON line
per figure.
  kernel   the pass alone on [batch][points][2] voltages and [batch][points][2] currents of device memory (512 x 4099 by
           default): 4 requests — v i with and without a reference node, v v, i i; HIP-event time of --calls calls back to
           back (each with its table upload) divided by their number, best of --reps after a warm-up
  passes   --variants variants of boost_probe as the instances of ONE handle, its own step count: Handle.run_measure_power
           with 4 stats requests and 4 product requests (switch, diode, source, load); the HIP-event times of the two
           passes (spicey_last_measure_ms, spicey_last_power_ms) and of the transient kernel, minimum of --rounds
  batch    measureTRANBatch with those 4 power() specs against the path without the pass — simulateTRANBatch, every
           waveform back on the host, then the products and their trapezoids by numpy — on the same variants, alternating
           order (wall s, parsing excluded)"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from batch_variants import variant  # noqa: E402
from conftest import golden_netlist, load_golden  # noqa: E402
from spicey_amd import abi, lib  # noqa: E402
from spicey_amd.batch import simulateTRANBatch  # noqa: E402
from spicey_amd.measure import _Plan, make_power_reqs, measureTRANBatch, power, reduce_reference_power, stats  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402

SOURCE = "Vsimulation_voltage_source_0"
POWER = {"sw": power("SM1"), "d": power("DD1"), "in": power(SOURCE), "load": power("RR1")}
STATS = {"n1": stats("v(n1)"), "n2": stats("v(n2)"), "n3": stats("v(n3)"), "il": stats("i(LL1)")}
trapz = getattr(np, "trapezoid", None) or np.trapz


def timed(call, reps, calls):
    """ms per call: `calls` of them between one pair of events, best of `reps` after a warm-up round."""
    import torch
    best = None
    for rep in range(reps + 1):  # (the first round is the warm-up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        if rep > 0:
            ms = e0.elapsed_time(e1) / calls
            best = ms if best is None else min(best, ms)
    return best


def kernel_case(batch, points, reps, calls):
    import torch
    dev = torch.device("cuda:0")
    d_v = torch.randn((batch, points, 2), dtype=torch.float64, device=dev)
    d_i = torch.randn((batch, points, 2), dtype=torch.float64, device=dev)
    reqs = make_power_reqs([(0, 0, -1, 1, 0, -1, 0, 0, -1), (0, 0, 1, 1, 1, -1, 1, 0, -1), (0, 0, -1, 0, 1, -1, 0, 0, -1), (1, 0, -1, 1, 1, -1, 0, 0, -1)])
    d_out = torch.empty((batch, len(reqs), abi.POWER_ROW), dtype=torch.float64, device=dev)
    nbytes = lib.power_workspace_bytes(batch, points, len(reqs))
    d_work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ms = timed(lambda: lib.power_device(batch, points, 1e-6, d_v.data_ptr(), 2, d_i.data_ptr(), 2, reqs, d_out.data_ptr(), d_work.data_ptr(), nbytes), reps, calls)
    # spot check: the device's numbers are the data's
    ref = reduce_reference_power(d_v[:1].cpu().numpy(), d_i[:1].cpu().numpy(), reqs, 1e-6)
    got = d_out[:1].cpu().numpy()
    free = [0, 1, 2, 3, 5, 6, 9, 10, 11, 12]
    assert np.array_equal(got[:, :, free], ref[:, :, free]) and np.allclose(got, ref, rtol=1e-10, atol=1e-12)
    loads = 2 + 4 + 2 + 2  # 8-byte loads per step of the four requests
    print(json.dumps(dict(case="kernel", n_inst=batch, points=points, requests=len(reqs), workspace_bytes=nbytes, calls_per_window=calls, ms=ms,
                          loaded_bytes_per_s=batch * points * loads * 8 / (ms * 1e-3))), flush=True)


def variants(n_var):
    # (without its .PRINT card: the path without the pass needs every node's waveform back, the measures ignore the card)
    base = "\n".join(ln for ln in golden_netlist(load_golden("boost_probe")).splitlines() if not ln.upper().startswith(".PRINT")) + "\n"
    return [variant(base, k / 16) for k in range(n_var)]


def passes_case(n_var, rounds):
    ckts = [parseNetlist(t) for t in variants(n_var)]
    tran = ckts[0].analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tran["dt"], tran["tstop"])
    plans = [_Plan(c, {**STATS, **POWER}, dt, steps) for c in ckts]
    assert all(p.key() == plans[0].key() for p in plans) and len(plans[0].reqs) == 4 and len(plans[0].preqs) == 4
    flat = abi.stack_instances([p.flatten(c) for p, c in zip(plans, ckts)])
    tabs = abi.source_tables(ckts, dt, steps)
    power_ms, measure_ms, kernel_ms = [], [], []
    for _ in range(rounds + 1):  # (the first round is the warm-up)
        h = lib.Handle(flat)
        try:
            res = h.run_measure_power(steps, dt, tabs, plans[0].reqs, [], [], [], plans[0].preqs, want_iters=False)
            assert res["status"] == 0, res["detail"]
            power_ms.append(res["power_ms"])
            measure_ms.append(res["measure_ms"])
            kernel_ms.append(res["kernel_ms"])
        finally:
            h.close()
    print(json.dumps(dict(case="passes", circuit="boost_probe", variants=n_var, points=steps + 1, recorded_nodes=int(flat.n_out), currents=int(flat.n_cur),
                          stats_requests=4, power_requests=4, power_ms=min(power_ms[1:]), measure_ms=min(measure_ms[1:]), kernel_ms=min(kernel_ms[1:]),
                          power_ms_all=power_ms[1:], measure_ms_all=measure_ms[1:])), flush=True)


def batch_case(n_var, rounds):
    texts = variants(n_var)
    t_meas, t_sim = [], []
    for rnd in range(rounds):
        for which in (("measure", "simulate") if rnd % 2 == 0 else ("simulate", "measure")):
            ckts = [parseNetlist(t) for t in texts]
            t0 = time.perf_counter()
            if which == "measure":
                got = measureTRANBatch(ckts, POWER)
                t_meas.append(time.perf_counter() - t0)
            else:
                res = simulateTRANBatch(ckts)
                ref = []
                for r in res:  # the same numbers from the returned lists
                    v, i = r["nodeVoltages"], r["elementCurrents"]
                    dt = r["times"][1]
                    n2, n3 = np.asarray(v["N2"]), np.asarray(v["N3"])
                    ref.append([float(trapz(p, dx=dt)) for p in (n2 * np.asarray(i["SM1"]), (n2 - n3) * np.asarray(i["DD1"]),
                                                                 np.asarray(v["N1"]) * np.asarray(i[SOURCE]), n3 * np.asarray(i["RR1"]))])
                t_sim.append(time.perf_counter() - t0)
    # (to the parity bar, relative to the energy the source delivered: the switch's own is a small difference)
    same = all(abs(g[k]["energy"] - e) <= 1e-9 * max(abs(e), abs(r[2])) for g, r in zip(got, ref) for k, e in zip(("sw", "d", "in", "load"), r))
    print(json.dumps(dict(case="batch", circuit="boost_probe", variants=n_var, mode="default", measureTRANBatch_s=min(t_meas),
                          simulateTRANBatch_numpy_s=min(t_sim), ratio=min(t_sim) / min(t_meas), measureTRANBatch_all_s=t_meas,
                          simulateTRANBatch_numpy_all_s=t_sim, same_numbers=bool(same))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--points", type=int, default=4099)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variants", type=int, default=256)
    ap.add_argument("--only", choices=["kernel", "passes", "batch"], default=None)
    a = ap.parse_args()
    if a.only in (None, "kernel"):
        kernel_case(a.batch, a.points, a.reps, a.calls)
    if a.only in (None, "passes"):
        passes_case(a.variants, a.rounds)
    if a.only in (None, "batch"):
        batch_case(a.variants, a.rounds)


if __name__ == "__main__":
    main()
