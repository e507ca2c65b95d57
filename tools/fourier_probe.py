#!/usr/bin/env python3
"""Cost of the device-side harmonics pass (spicey_fourier_device, Handle.run_measure_fourier), one JSON line per figure.
  kernel       the reduction alone on [batch][points][nodes] doubles of device memory (diode_chain(1000) x 512 x 1 001
               points by default, about 4.1 GB): 9 harmonics on every node, and on 2 recorded nodes; HIP-event time of both
               of its kernels (the table upload included), best of --reps after a warm-up; bytes of waveform read per
               second against 6.3 TB/s, and the ratio to the stats pass (spicey_measure_device, every column) on the same
               buffers in the same process
  end_to_end   Handle.run_measure_fourier against the path without it — Handle.run (waveforms copied to the host), then
               the same sums by numpy (one matrix product per instance) — on that workload, all nodes and two probes,
               alternating order (wall s)"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from spicey_amd import lib, synth  # noqa: E402
from spicey_amd.measure import make_four_reqs, make_reqs  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s


def four_reqs(n, harm, f0):
    return make_four_reqs([(0, c, -1, harm, 0, -1, f0) for c in range(n)])


def twiddle_matrix(points, harm, f0, dt):
    """[1 + 2 harm][points - 1]: the rows a sample vector is multiplied with (ones, c_1, s_1, ...), numpy's cos / sin."""
    s = np.arange(points - 1, dtype=np.int64)
    rows = [np.ones(points - 1)]
    for h in range(1, harm + 1):
        r = (h * s).astype(np.float64) * (f0 * dt)
        a = (2.0 * np.pi) * (r - np.floor(r))
        rows += [np.cos(a), np.sin(a)]
    return np.stack(rows)


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


def kernel_cases(nodes, batch, points, harm, reps):
    import torch
    dev = torch.device("cuda:0")
    dt = 1e-6
    f0 = 1.0 / (50 * dt)
    for label, n_v in (("all_nodes", nodes), ("two_probes", 2)):
        d_v = torch.rand((batch, points, n_v), dtype=torch.float64, device=dev)
        freqs = four_reqs(n_v, harm, f0)
        width = lib.fourier_row_doubles(freqs)
        d_out = torch.empty((batch, n_v, width), dtype=torch.float64, device=dev)
        nbytes = lib.fourier_workspace_bytes(batch, points, freqs)
        d_work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ms = timed(lambda: lib.fourier_device(batch, points, dt, d_v.data_ptr(), n_v, 0, 0, freqs, d_out.data_ptr(), width, d_work.data_ptr(), nbytes), reps)
        # the stats pass on the same buffers: the same bytes read once
        sreqs = make_reqs([(0, 0, c, -1, 0, -1, 0.0, 0) for c in range(n_v)])
        d_meas = torch.empty((batch, n_v, 8), dtype=torch.float64, device=dev)
        sbytes = lib.measure_workspace_bytes(batch, points, n_v)
        d_swork = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        stats_ms = timed(lambda: lib.measure_device(batch, points, dt, d_v.data_ptr(), n_v, 0, 0, sreqs, d_meas.data_ptr(), d_swork.data_ptr(), sbytes), reps)
        # spot check: the device's numbers are the data's
        row = d_out[0, n_v - 1].cpu().numpy()
        x = d_v[0, :points - 1, n_v - 1].cpu().numpy()
        want = twiddle_matrix(points, harm, f0, dt) @ x
        assert np.allclose(row, want, rtol=0, atol=1e-9 * np.abs(x).sum()), (row, want)
        read = batch * (points - 1) * n_v * 8
        print(json.dumps(dict(case="kernel", requests=label, harmonics=harm, n_inst=batch, points=points, columns=n_v, waveform_bytes=read,
                              workspace_bytes=nbytes, ms=ms, read_bytes_per_s=read / (ms * 1e-3), fraction_of_6p3_TBps=read / (ms * 1e-3) / HBM_ACHIEVABLE,
                              stats_ms=stats_ms, ratio_to_stats=ms / stats_ms)), flush=True)
        del d_v, d_out, d_work, d_meas, d_swork


def end_to_end(nodes, batch, points, harm, rounds):
    flat, dt, steps, src = synth.chain_batch("diode_chain", nodes, range(1, batch + 1), tran=f".tran 1e-6 {(points - 1.5) * 1e-6!r}")
    assert steps + 1 == points  # (a stop time half a step short of the last point: ceil gives points - 1 steps)
    f0 = 1.0 / (50 * dt)
    tw = twiddle_matrix(points, harm, f0, dt)
    for label, out_nodes in (("all_nodes", None), ("two_probes", [nodes // 2, nodes])):
        flat.out_nodes = None if out_nodes is None else np.ascontiguousarray(out_nodes, dtype=np.int32)
        freqs = four_reqs(flat.n_out, harm, f0)
        t_dev, t_host, kernel_ms, fourier_ms = [], [], [], []
        agree = True
        for rnd in range(rounds):
            for which in (("device", "host") if rnd % 2 == 0 else ("host", "device")):
                h = lib.Handle(flat)
                try:
                    t0 = time.perf_counter()
                    if which == "device":
                        res = h.run_measure_fourier(steps, dt, src, make_reqs([]), freqs, want_iters=False)
                        got = res["four"]
                        t_dev.append(time.perf_counter() - t0)
                        kernel_ms.append(res["kernel_ms"])
                        fourier_ms.append(res["fourier_ms"])
                    else:
                        res = h.run(steps, dt, src, want_currents=False, want_iters=False)
                        ref = np.stack([(tw @ res["out_v"][i, :points - 1]).T for i in range(batch)])
                        t_host.append(time.perf_counter() - t0)
                    assert res["status"] == 0, res["detail"]
                finally:
                    h.close()
                del res
            scale = np.abs(ref[:, :, 0]).max() + (points - 1)
            agree = agree and bool(np.abs(got - ref).max() <= 1e-9 * scale)
        print(json.dumps(dict(case="end_to_end", requests=label, harmonics=harm, n_inst=batch, points=points, recorded_nodes=flat.n_out,
                              run_measure_fourier_s=min(t_dev), run_then_numpy_s=min(t_host), ratio=min(t_host) / min(t_dev),
                              run_measure_fourier_all_s=t_dev, run_then_numpy_all_s=t_host, kernel_ms=min(kernel_ms), fourier_ms=min(fourier_ms),
                              same_numbers=bool(agree))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--points", type=int, default=1001)
    ap.add_argument("--harmonics", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=["kernel", "end_to_end"], default=None)
    a = ap.parse_args()
    if a.only in (None, "kernel"):
        kernel_cases(a.nodes, a.batch, a.points, a.harmonics, a.reps)
    if a.only in (None, "end_to_end"):
        end_to_end(a.nodes, a.batch, a.points, a.harmonics, a.rounds)


if __name__ == "__main__":
    main()
