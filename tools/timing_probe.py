#!/usr/bin/env python3
"""Cost of the device-side edge-timing pass (spicey_timing_device, measureTRANBatch with when / delay), one JSON line per figure.
  kernel       the pass alone on [batch][points][nodes] doubles of device memory (512 x 1 001 x 1 000 by default, about
               4.1 GB): one when() per column, on every column and on two; with an absolute level (the two kernels of this
               pass alone) and with rel(0.5) (the base windows through the measurement pass first); HIP-event time, the
               table uploads included, best of --reps after a warm-up; beside it the measurement pass's cross() and stats()
               on the same buffers in the same process, and the ratio to cross()
  end_to_end   measureTRANBatch with a delay and a rise time on --variants supply-scaled half bridges against the path
               without the pass — simulateTRANBatch (every sample to the host), then reduce_reference_timing on its lists —
               alternating order, minimum of --rounds (wall s); same_numbers: both routes give the same dicts, compared by =="""
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
from spicey_amd import abi, lib  # noqa: E402
from spicey_amd import measure as M  # noqa: E402
from spicey_amd.batch import simulateTRANBatch  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s

def timed(call, reps):
    import torch
    best = None
    for rep in range(reps + 1):  # (the first run is the warm-up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if rep > 0:
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
    return best


def kernel_cases(nodes, batch, points, reps):
    import torch
    dev = torch.device("cuda:0")
    dt = 1e-6
    for label, n_v in (("all_nodes", nodes), ("two_probes", 2)):
        d_v = torch.rand((batch, points, n_v), dtype=torch.float64, device=dev)
        d_out = torch.empty((batch, n_v, 8), dtype=torch.float64, device=dev)
        fig = {}
        for name, kind in (("abs", abi.TIMING_ABS), ("rel", abi.TIMING_MINMAX)):
            treqs = M.make_timing_reqs([(0, -1, None, (0, c, -1, 1, 3, kind, 0, -1, 0.5), 0) for c in range(n_v)])  # the 3rd rise through 0.5
            nbytes = lib.timing_workspace_bytes(batch, points, treqs)
            d_work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            fig[name + "_ms"] = timed(lambda: lib.timing_device(batch, points, dt, d_v.data_ptr(), n_v, 0, 0, treqs, d_out.data_ptr(), d_work.data_ptr(), nbytes), reps)
            fig[name + "_workspace_bytes"] = nbytes
            # spot check: the device's rows are the data's
            got = d_out[:2].cpu().numpy()
            want = M.reduce_reference_timing(d_v[:2].cpu().numpy(), None, treqs, dt)
            assert (got.view(np.int64) == want.view(np.int64)).all() and (want[:, :, 3] >= 0).all()
            del d_work
        # the measurement pass on the same buffers: the same bytes read once
        d_meas = torch.empty((batch, n_v, 8), dtype=torch.float64, device=dev)
        sbytes = lib.measure_workspace_bytes(batch, points, n_v)
        d_swork = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        for name, row in (("cross", lambda c: (1, 0, c, -1, 0, -1, 0.5, 1)), ("stats", lambda c: (0, 0, c, -1, 0, -1, 0.0, 0))):
            sreqs = M.make_reqs([row(c) for c in range(n_v)])
            fig[name + "_ms"] = timed(lambda: lib.measure_device(batch, points, dt, d_v.data_ptr(), n_v, 0, 0, sreqs, d_meas.data_ptr(), d_swork.data_ptr(), sbytes), reps)
        read = batch * points * n_v * 8
        print(json.dumps(dict(case="kernel", requests=label, n_inst=batch, points=points, columns=n_v, waveform_bytes=read, **fig,
                              abs_read_bytes_per_s=read / (fig["abs_ms"] * 1e-3), abs_fraction_of_6p3_TBps=read / (fig["abs_ms"] * 1e-3) / HBM_ACHIEVABLE,
                              abs_ratio_to_cross=fig["abs_ms"] / fig["cross_ms"], rel_ratio_to_cross=fig["rel_ms"] / fig["cross_ms"])), flush=True)
        del d_v, d_out, d_meas, d_swork


def end_to_end(variants, rounds):
    base = golden_netlist(load_golden("half_bridge"))
    assert base.count("dc 12") == 1
    texts = [base.replace("dc 12", f"dc {12.0 * (1 + 0.002 * k)!r}") for k in range(variants)]  # the supply scaled: every variant another level
    m = {"d": M.delay(trig=M.edge("v(g1)", M.rel(0.5)), targ=M.edge("v(sw)", M.rel(0.5))), "r": M.rise_time("v(out)")}
    t_dev, t_host = [], []
    agree = True
    for rnd in range(rounds):
        for which in (("device", "host") if rnd % 2 == 0 else ("host", "device")):
            ckts = [parseNetlist(t) for t in texts]
            t0 = time.perf_counter()
            if which == "device":
                got = M.measureTRANBatch(ckts, m, diagnostics=False)
                t_dev.append(time.perf_counter() - t0)
            else:
                res = simulateTRANBatch(ckts, diagnostics=False)
                ref = []
                for c, r in zip(ckts, res):
                    dt, steps = abi.computeEffectiveTimeStep(c.analyses["tran"]["dt"], c.analyses["tran"]["tstop"])
                    plan = M._Plan(c, m, dt, steps)
                    v = np.stack([np.asarray(r["nodeVoltages"][c.nodes.rev[n]], dtype=np.float64) for n in plan.out_nodes], axis=1)[None]
                    ref.append(plan.values({"timing": M.reduce_reference_timing(v, None, plan.treqs, dt)}, 0, dt))
                t_host.append(time.perf_counter() - t0)
        agree = agree and got == ref  # (every value, None included, by ==: the same bits)
    print(json.dumps(dict(case="end_to_end", circuit="half_bridge", variants=variants, measureTRANBatch_s=min(t_dev), simulate_then_numpy_s=min(t_host),
                          ratio=min(t_host) / min(t_dev), measureTRANBatch_all_s=t_dev, simulate_then_numpy_all_s=t_host, same_numbers=bool(agree),
                          delay_of_variant_0=got[0]["d"]["delay"], rise_time_of_variant_0=got[0]["r"]["time"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--points", type=int, default=1001)
    ap.add_argument("--variants", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=["kernel", "end_to_end"], default=None)
    a = ap.parse_args()
    if a.only in (None, "kernel"):
        kernel_cases(a.nodes, a.batch, a.points, a.reps)
    if a.only in (None, "end_to_end"):
        end_to_end(a.variants, a.rounds)


if __name__ == "__main__":
    main()
