#!/usr/bin/env python3
"""Cost of the device-side waveform measurements (spicey_measure_device, Handle.run_measure, measureTRANBatch), one JSON
line per figure.
  kernel       the reduction alone on [batch][points][nodes] doubles of device memory (diode_chain(1000) x 512 x 1 001
               points by default, about 4.1 GB): stats on every node, and 2 requests on 2 recorded nodes; HIP-event time of
               both of its kernels, best of --reps after a warm-up; bytes of waveform read per second against 6.3 TB/s
  end_to_end   Handle.run_measure against the path without it — Handle.run (waveforms copied to the host), then the same
               numbers by numpy reductions — on that workload, all nodes and two probes, alternating order (wall s)
  batch        measureTRANBatch against simulateTRANBatch plus numpy on --variants variants of boost_probe (wall s,
               parsing excluded), alternating order"""
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
from spicey_amd import lib, synth  # noqa: E402
from spicey_amd.batch import simulateTRANBatch  # noqa: E402
from spicey_amd.measure import cross, make_reqs, measureTRANBatch, stats  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s


def stats_reqs(n):
    return make_reqs([(0, 0, c, -1, 0, -1, 0.0, 0) for c in range(n)])


def kernel_cases(nodes, batch, points, reps):
    import torch
    dev = torch.device("cuda:0")
    for label, n_v in (("all_nodes", nodes), ("two_probes", 2)):
        d_v = torch.rand((batch, points, n_v), dtype=torch.float64, device=dev)
        reqs = stats_reqs(n_v)
        d_meas = torch.empty((batch, n_v, 8), dtype=torch.float64, device=dev)
        nbytes = lib.measure_workspace_bytes(batch, points, n_v)
        d_work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        best = None
        for rep in range(reps + 1):  # (the first run is the warm-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lib.measure_device(batch, points, 1e-6, d_v.data_ptr(), n_v, 0, 0, reqs, d_meas.data_ptr(), d_work.data_ptr(), nbytes)
            e1.record()
            torch.cuda.synchronize()
            if rep > 0:
                ms = e0.elapsed_time(e1)
                best = ms if best is None else min(best, ms)
        # spot check: the device's numbers are the data's
        m = d_meas[0, n_v - 1].cpu().numpy()
        x = d_v[0, :, n_v - 1].cpu().numpy()
        assert m[0] == x.min() and m[1] == x.max() and m[6] == x[0] and m[7] == x[-1] and abs(m[4] - x.sum()) <= 1e-9 * x.sum()
        read = batch * points * n_v * 8
        print(json.dumps(dict(case="kernel", requests=label, n_inst=batch, points=points, columns=n_v, waveform_bytes=read,
                              workspace_bytes=nbytes, ms=best, read_bytes_per_s=read / (best * 1e-3),
                              fraction_of_6p3_TBps=read / (best * 1e-3) / HBM_ACHIEVABLE)), flush=True)
        del d_v, d_meas, d_work


def numpy_stats(out_v):
    """The 8 numbers of stats on every column of out_v [n_inst][points][n], as numpy gives them."""
    mn, mx = out_v.min(axis=1), out_v.max(axis=1)
    amn, amx = out_v.argmin(axis=1), out_v.argmax(axis=1)
    s = out_v.sum(axis=1)
    sq = np.einsum("ipn,ipn->in", out_v, out_v)
    return np.stack([mn, mx, amn.astype(np.float64), amx.astype(np.float64), s, sq, out_v[:, 0], out_v[:, -1]], axis=2)


def end_to_end(nodes, batch, points, rounds):
    flat, dt, steps, src = synth.chain_batch("diode_chain", nodes, range(1, batch + 1), tran=f".tran 1e-6 {(points - 1.5) * 1e-6!r}")
    assert steps + 1 == points  # (a stop time half a step short of the last point: ceil gives points - 1 steps)
    for label, out_nodes in (("all_nodes", None), ("two_probes", [nodes // 2, nodes])):
        flat.out_nodes = None if out_nodes is None else np.ascontiguousarray(out_nodes, dtype=np.int32)
        reqs = stats_reqs(flat.n_out)
        t_meas, t_host, kernel_ms, measure_ms = [], [], [], []
        agree = True
        for rnd in range(rounds):
            for which in (("measure", "host") if rnd % 2 == 0 else ("host", "measure")):
                h = lib.Handle(flat)
                try:
                    t0 = time.perf_counter()
                    if which == "measure":
                        res = h.run_measure(steps, dt, src, reqs, want_iters=False)
                        got = res["meas"]
                        t_meas.append(time.perf_counter() - t0)
                        kernel_ms.append(res["kernel_ms"])
                        measure_ms.append(res["measure_ms"])
                    else:
                        res = h.run(steps, dt, src, want_currents=False, want_iters=False)
                        ref = numpy_stats(res["out_v"])
                        t_host.append(time.perf_counter() - t0)
                    assert res["status"] == 0, res["detail"]
                finally:
                    h.close()
                del res
            agree = agree and np.array_equal(got[:, :, [0, 1, 2, 3, 6, 7]], ref[:, :, [0, 1, 2, 3, 6, 7]]) and np.allclose(got, ref, rtol=1e-12, atol=0)
        print(json.dumps(dict(case="end_to_end", requests=label, n_inst=batch, points=points, recorded_nodes=flat.n_out,
                              run_measure_s=min(t_meas), run_then_numpy_s=min(t_host), ratio=min(t_host) / min(t_meas),
                              run_measure_all_s=t_meas, run_then_numpy_all_s=t_host, kernel_ms=min(kernel_ms), measure_ms=min(measure_ms),
                              same_numbers=bool(agree))), flush=True)


def batch_case(n_var, rounds):
    base = golden_netlist(load_golden("boost_probe"))
    texts = [variant(base, k / 16) for k in range(n_var)]
    m = {"peak": stats("v(n3)"), "ripple": stats("v(n3)", t_from=0.05), "il": stats("i(LL1)"), "up": cross("v(n3)", 5.0, dir="rise")}
    for exact in (False, True):
        t_meas, t_sim = [], []
        for rnd in range(rounds):
            for which in (("measure", "simulate") if rnd % 2 == 0 else ("simulate", "measure")):
                ckts = [parseNetlist(t) for t in texts]
                t0 = time.perf_counter()
                if which == "measure":
                    got = measureTRANBatch(ckts, m, exact_order=exact)
                    t_meas.append(time.perf_counter() - t0)
                else:
                    res = simulateTRANBatch(ckts, exact_order=exact)
                    ref = []
                    for r in res:  # the same numbers from the returned lists
                        v = np.asarray(r["nodeVoltages"]["N3"])
                        il = np.asarray(r["elementCurrents"]["LL1"])
                        up = np.nonzero((v[:-1] < 5.0) & (v[1:] >= 5.0))[0]
                        ref.append((v.min(), v.max(), v[50:].min(), v[50:].max(), il.sum(), len(up)))
                    t_sim.append(time.perf_counter() - t0)
        same = all(g["peak"]["max"] == r[1] and g["ripple"]["min"] == r[2] and g["up"]["count"] == r[5] for g, r in zip(got, ref)) if not exact else \
            all((g["peak"]["min"], g["peak"]["max"], g["ripple"]["min"], g["ripple"]["max"], g["up"]["count"]) == (r[0], r[1], r[2], r[3], r[5]) for g, r in zip(got, ref))
        print(json.dumps(dict(case="batch", circuit="boost_probe", variants=n_var, mode="exact" if exact else "default",
                              measureTRANBatch_s=min(t_meas), simulateTRANBatch_numpy_s=min(t_sim), ratio=min(t_sim) / min(t_meas),
                              measureTRANBatch_all_s=t_meas, simulateTRANBatch_numpy_all_s=t_sim, same_numbers=bool(same))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--points", type=int, default=1001)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--variants", type=int, default=256)
    ap.add_argument("--only", choices=["kernel", "end_to_end", "batch"], default=None)
    a = ap.parse_args()
    if a.only in (None, "kernel"):
        kernel_cases(a.nodes, a.batch, a.points, a.reps)
    if a.only in (None, "end_to_end"):
        end_to_end(a.nodes, a.batch, a.points, a.rounds)
    if a.only in (None, "batch"):
        batch_case(a.variants, a.rounds)


if __name__ == "__main__":
    main()
