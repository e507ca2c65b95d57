#!/usr/bin/env python3
"""Cost of the device-side spectrum pass (spicey_spectrum_device, Handle.run_measure_spectrum), one JSON line per figure.
  kernel       the pass alone on [batch][points][2] doubles of device memory (512 x 4099 x 2 by default), two requests of
               N = 4096, one per column: as dominant() and as a full-band spectrum(); HIP-event time of --calls calls
               back to back (each with its table upload) divided by their number, best of --reps after a warm-up;
               transforms per second and the bytes of waveform gathered per second
  end_to_end   Handle.run_measure_spectrum against the path without it — Handle.run (waveforms copied to the host), then
               numpy.fft.rfft of the same Hann-windowed samples — on a diode chain with two recorded nodes, alternating
               order, minimum of the rounds (wall s)"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from spicey_amd import abi, lib, synth  # noqa: E402
from spicey_amd.measure import make_reqs, make_spec_reqs, spectrum_tables  # noqa: E402


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


def kernel_cases(batch, points, log2n, reps, calls):
    import torch
    dev = torch.device("cuda:0")
    dt, N = 1e-6, 1 << log2n
    s0 = points - N
    d_v = torch.randn((batch, points, 2), dtype=torch.float64, device=dev)
    for label, kind in (("dominant", abi.SPEC_DOMINANT), ("spectrum_full_band", abi.SPEC_BINS)):
        reqs = make_spec_reqs([(0, c, -1, kind, s0, log2n, abi.SPEC_HANN, 1 if kind else 0, N // 2) for c in range(2)])
        width = abi.spec_row_doubles(reqs)
        d_out = torch.empty((batch, 2, width), dtype=torch.float64, device=dev)
        nbytes = lib.spectrum_workspace_bytes(batch, points, reqs)
        d_work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ms = timed(lambda: lib.spectrum_device(batch, points, dt, d_v.data_ptr(), 2, 0, 0, reqs, d_out.data_ptr(), width, d_work.data_ptr(), nbytes), reps, calls)
        # spot check: the device's numbers are the data's
        x = d_v[0, s0:, 1].cpu().numpy()
        X = np.fft.rfft(x * spectrum_tables(log2n)[2])
        row = d_out[0, 1].cpu().numpy()
        tol = 1e-9 * np.abs(x).sum()
        if kind == abi.SPEC_BINS:
            assert np.abs(row[0::2] - X.real).max() <= tol and np.abs(row[1::2] - X.imag).max() <= tol
        else:
            assert int(row[0]) == 1 + int(np.argmax(np.abs(X[1:]))) and abs(row[1] + 1j * row[2] - X[int(row[0])]) <= tol
        items = batch * 2
        print(json.dumps(dict(case="kernel", requests=label, n_inst=batch, points=points, n=N, items=items, lds_bytes=16 * N, workspace_bytes=nbytes,
                              row_doubles=width, calls_per_window=calls, ms=ms, transforms_per_s=items / (ms * 1e-3), gathered_bytes_per_s=items * N * 8 / (ms * 1e-3))), flush=True)
        del d_out, d_work


def end_to_end(nodes, batch, points, log2n, rounds):
    flat, dt, steps, src = synth.chain_batch("diode_chain", nodes, range(1, batch + 1), tran=f".tran 1e-6 {(points - 1.5) * 1e-6!r}")
    assert steps + 1 == points  # (a stop time half a step short of the last point: ceil gives points - 1 steps)
    N = 1 << log2n
    s0 = points - N
    flat.out_nodes = np.ascontiguousarray([nodes // 2, nodes], dtype=np.int32)
    sreqs = make_spec_reqs([(0, c, -1, abi.SPEC_BINS, s0, log2n, abi.SPEC_HANN, 0, N // 2) for c in range(2)])
    w = spectrum_tables(log2n)[2]
    t_dev, t_host, kernel_ms, spectrum_ms = [], [], [], []
    agree = True
    for rnd in range(rounds):
        for which in (("device", "host") if rnd % 2 == 0 else ("host", "device")):
            h = lib.Handle(flat)
            try:
                t0 = time.perf_counter()
                if which == "device":
                    res = h.run_measure_spectrum(steps, dt, src, make_reqs([]), [], [], sreqs, want_iters=False)
                    got = res["spec"][:, :, 0::2] + 1j * res["spec"][:, :, 1::2]
                    t_dev.append(time.perf_counter() - t0)
                    kernel_ms.append(res["kernel_ms"])
                    spectrum_ms.append(res["spectrum_ms"])
                else:
                    res = h.run(steps, dt, src, want_currents=False, want_iters=False)
                    ref = np.fft.rfft(res["out_v"][:, s0:, :] * w[None, :, None], axis=1).transpose(0, 2, 1)
                    t_host.append(time.perf_counter() - t0)
                assert res["status"] == 0, res["detail"]
            finally:
                h.close()
            del res
        agree = agree and bool(np.abs(got - ref).max() <= 1e-9 * (np.abs(ref).max() + N))
    print(json.dumps(dict(case="end_to_end", n_inst=batch, nodes=nodes, points=points, n=N, recorded_nodes=2,
                          run_measure_spectrum_s=min(t_dev), run_then_numpy_s=min(t_host), ratio=min(t_host) / min(t_dev),
                          run_measure_spectrum_all_s=t_dev, run_then_numpy_all_s=t_host, kernel_ms=min(kernel_ms), spectrum_ms=min(spectrum_ms),
                          same_numbers=bool(agree))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--points", type=int, default=4099)
    ap.add_argument("--log2n", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["kernel", "end_to_end"], default=None)
    a = ap.parse_args()
    if a.only in (None, "kernel"):
        kernel_cases(a.batch, a.points, a.log2n, a.reps, a.calls)
    if a.only in (None, "end_to_end"):
        end_to_end(a.nodes, a.batch, a.points, a.log2n, a.rounds)


if __name__ == "__main__":
    main()
