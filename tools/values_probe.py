#!/usr/bin/env python3
"""Cost of the device-side values pass (spicey_values_device, Handle.run_reduced, trace() / sample() / find()), one JSON line
per figure.
  kernel   the pass alone on [batch][points][4] voltages of device memory (64 x 100001 by default): 4 traces of 512 buckets,
           one run of 1000 points and one find; HIP-event time of --calls calls back to back (each with its head upload
           and the clear of the rows) divided by their number, best of --reps after a warm-up
  passes   --variants variants of boost_probe as the instances of ONE handle, --steps steps (default: the circuit's own):
           Handle.run_reduced with 4 stats requests, one hidden timing request and 4 traces of 512 buckets plus one find;
           the HIP-event times of the passes (spicey_last_measure_ms, spicey_last_timing_ms, spicey_last_values_ms) and of
           the transient kernel, minimum of --rounds, and the bytes of results that came back
  batch    measureTRANBatch with those trace() / find() specs against the path without the pass — simulateTRANBatch, every
           waveform back on the host, then reduce_reference_timing and reduce_reference_values — on the same variants,
           alternating order (wall s, parsing excluded), and the bytes either path brings back"""
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
from spicey_amd.measure import (_Plan, edge, find, make_timing_reqs, make_value_points, make_value_reqs, measureTRANBatch, reduce_reference_timing,  # noqa: E402
                                reduce_reference_values, rel, stats, trace)
from spicey_amd.netlist import parseNetlist  # noqa: E402

VALUES = {"n1": trace("v(n1)"), "n2": trace("v(n2)"), "n3": trace("v(n3)"), "il": trace("i(LL1)"),
          "valley": find("i(LL1)", when=edge("v(n2)", rel(0.5), "rise"))}
STATS = {"s1": stats("v(n1)"), "s2": stats("v(n2)"), "s3": stats("v(n3)"), "sl": stats("i(LL1)")}


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
    d_v = torch.randn((batch, points, 4), dtype=torch.float64, device=dev)
    treqs = make_timing_reqs([(0, -1, None, (0, 0, -1, 1, 1, abi.TIMING_ABS, 0, 0, 0.25), 0)])
    rng = np.random.default_rng(0)
    pts = make_value_points(list(zip(rng.integers(0, points - 1, 1000).tolist(), rng.random(1000).tolist())))
    reqs = make_value_reqs([(0, 0, c, -1, 0, 0, -1, 0, 0, -1, 0, 0, 512) for c in range(4)]
                           + [(1, 0, 1, -1, 0, 0, -1, 0, 0, 0, 0, 1000, 0), (2, 0, 1, -1, 0, 0, -1, 0, 0, 0, 0, 0, 0)])
    d_t = torch.empty((batch, 1, 8), dtype=torch.float64, device=dev)
    wt = lib.timing_workspace_bytes(batch, points, treqs)
    d_wt = torch.empty(wt, dtype=torch.uint8, device=dev)
    lib.timing_device(batch, points, 1e-6, d_v.data_ptr(), 4, 0, 0, treqs, d_t.data_ptr(), d_wt.data_ptr(), wt)
    stride = abi.val_row_doubles(reqs)
    d_out = torch.empty((batch, len(reqs), stride), dtype=torch.float64, device=dev)
    nbytes = lib.values_workspace_bytes(batch, points, reqs, len(pts))
    d_work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ms = timed(lambda: lib.values_device(batch, points, 1e-6, d_v.data_ptr(), 4, 0, 0, reqs, pts, d_t.data_ptr(), 1, d_out.data_ptr(), stride, d_work.data_ptr(),
                                         nbytes), reps, calls)
    # spot check: the device's numbers are the data's, bit for bit
    ref = reduce_reference_values(d_v[:1].cpu().numpy(), None, reqs, pts, 1e-6, d_t[:1].cpu().numpy())
    assert np.array_equal(d_out[:1].cpu().numpy().view(np.int64), ref.view(np.int64))
    print(json.dumps(dict(case="kernel", n_inst=batch, points=points, requests=len(reqs), workspace_bytes=nbytes, result_bytes=d_out.numel() * 8,
                          calls_per_window=calls, ms=ms, loaded_bytes_per_s=batch * points * 4 * 8 / (ms * 1e-3))), flush=True)


def variants(n_var, steps):
    # (without its .PRINT card: the path without the pass needs every node's waveform back, the measures ignore the card)
    base = "\n".join(ln for ln in golden_netlist(load_golden("boost_probe")).splitlines() if not ln.upper().startswith(".PRINT")) + "\n"
    if steps:
        assert ".tran 0.001 0.1 uic" in base
        base = base.replace(".tran 0.001 0.1 uic", f".tran {0.1 / steps!r} 0.1 uic")
    return [variant(base, k / 16) for k in range(n_var)]


def passes_case(n_var, rounds, steps):
    ckts = [parseNetlist(t) for t in variants(n_var, steps)]
    tran = ckts[0].analyses["tran"]
    dt, steps = abi.computeEffectiveTimeStep(tran["dt"], tran["tstop"])
    plans = [_Plan(c, {**STATS, **VALUES}, dt, steps) for c in ckts]
    p0 = plans[0]
    assert all(p.key() == p0.key() for p in plans) and len(p0.reqs) == 4 and len(p0.vreqs) == 5 and len(p0.treqs) == 1
    flat = abi.stack_instances([p.flatten(c) for p, c in zip(plans, ckts)])
    tabs = abi.source_tables(ckts, dt, steps)
    ms = {k: [] for k in ("values_ms", "measure_ms", "timing_ms", "kernel_ms")}
    for _ in range(rounds + 1):  # (the first round is the warm-up)
        h = lib.Handle(flat)
        try:
            res = h.run_reduced(steps, dt, tabs, reqs=p0.reqs, treqs=p0.treqs, vreqs=p0.vreqs, pts=p0.pts, want_iters=False)
            assert res["status"] == 0, res["detail"]
            for k in ms:
                ms[k].append(res[k])
        finally:
            h.close()
    back = sum(res[k].nbytes for k in ("meas", "timing", "values"))
    print(json.dumps(dict(case="passes", circuit="boost_probe", variants=n_var, points=steps + 1, recorded_nodes=int(flat.n_out), currents=int(flat.n_cur),
                          stats_requests=4, traces=4, buckets=int(p0.vreqs[0]["buckets"]), finds=1, result_bytes=back,
                          waveform_bytes=n_var * (steps + 1) * (int(flat.n_out) + int(flat.n_cur)) * 8,
                          **{k: min(v[1:]) for k, v in ms.items()}, values_ms_all=ms["values_ms"][1:], measure_ms_all=ms["measure_ms"][1:])), flush=True)


def batch_case(n_var, rounds, steps):
    texts = variants(n_var, steps)
    t_meas, t_sim = [], []
    for rnd in range(rounds):
        for which in (("measure", "simulate") if rnd % 2 == 0 else ("simulate", "measure")):
            ckts = [parseNetlist(t) for t in texts]
            t0 = time.perf_counter()
            if which == "measure":
                got = measureTRANBatch(ckts, VALUES)
                t_meas.append(time.perf_counter() - t0)
            else:
                res = simulateTRANBatch(ckts)
                # the same answers from the returned waveforms: the numpy definitions of the two passes
                dt = float(res[0]["times"][1])
                out_v = np.stack([np.stack([np.asarray(r["nodeVoltages"][n]) for n in ("N1", "N2", "N3")], axis=1) for r in res])
                out_i = np.stack([np.asarray(r["elementCurrents"]["LL1"])[:, None] for r in res])
                treqs = make_timing_reqs([(0, -1, None, (0, 1, -1, 1, 1, abi.TIMING_MINMAX, 0, -1, 0.5), 0)])
                B = min(512, out_v.shape[1])
                vreqs = make_value_reqs([(0, 0, c, -1, 0, 0, -1, 0, 0, -1, 0, 0, B) for c in range(3)] + [(0, 1, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, B),
                                                                                                          (2, 1, 0, -1, 0, 1, -1, 0, 0, 0, 0, 0, 0)])
                ref = reduce_reference_values(out_v, out_i, vreqs, [], dt, reduce_reference_timing(out_v, out_i, treqs, dt))
                t_sim.append(time.perf_counter() - t0)
                wave_bytes = sum(8 * len(a) for r in res for grp in ("nodeVoltages", "elementCurrents") for a in r[grp].values())
    # (the default engine against itself: the same launch geometry gives the same samples, so the same bits)
    same = all(g["n3"]["max"] == ref[k, 2, 2:6 * B:6].tolist() and g["valley"]["value"] == (ref[k, 4, 2] if ref[k, 4, 0] >= 0 else None) for k, g in enumerate(got))
    print(json.dumps(dict(case="batch", circuit="boost_probe", variants=n_var, points=int(out_v.shape[1]), mode="default", measureTRANBatch_s=min(t_meas),
                          simulateTRANBatch_numpy_s=min(t_sim), ratio=min(t_sim) / min(t_meas), measureTRANBatch_all_s=t_meas,
                          simulateTRANBatch_numpy_all_s=t_sim, waveform_bytes_back=int(wave_bytes), result_bytes_back=int(n_var * 5 * 6 * B * 8),
                          same_numbers=bool(same))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--points", type=int, default=100001)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variants", type=int, default=256)
    ap.add_argument("--steps", type=int, default=0, help="steps of the boost_probe runs (0: the circuit's own 100)")
    ap.add_argument("--only", choices=["kernel", "passes", "batch"], default=None)
    a = ap.parse_args()
    if a.only in (None, "kernel"):
        kernel_case(a.batch, a.points, a.reps, a.calls)
    if a.only in (None, "passes"):
        passes_case(a.variants, a.rounds, a.steps)
    if a.only in (None, "batch"):
        batch_case(a.variants, a.rounds, a.steps)


if __name__ == "__main__":
    main()
