#!/usr/bin/env python3
"""Cost of per-instance source tables (spicey_run_src) and of the batch front end (simulateTRANBatch), one JSON line each.
  kernel       diode_chain(1000) x 512 x 10 000 steps, the bench's workload: one shared table, per-instance tables whose rows
               are all equal, per-instance tables with distinct amplitudes (kernel ms, HIP events, best of --reps)
  end_to_end   256 variants of boost_probe (R, C and the pulse amplitude varied): simulateTRANBatch against a loop of
               simulateTRAN, default and exact mode (wall s, parsing excluded)"""
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
from spicey_amd import synth  # noqa: E402
from spicey_amd.batch import simulateTRANBatch  # noqa: E402
from spicey_amd.lib import Handle  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402
from spicey_amd.simulate import simulateTRAN  # noqa: E402


def kernel_cases(n, batch, steps, reps):
    import torch  # (device buffers as bench.py allocates them: the results of 512 x 10 000 steps do not fit a host copy)
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)  # (torch's HIP runtime first, as in bench.py)
    flat, dt, st, src = synth.chain_batch("diode_chain", n, range(1, batch + 1), tran=f".tran 1e-6 {steps * 1e-6!r}")
    tables = {"shared": src, "per_instance_equal": np.ascontiguousarray(np.broadcast_to(src, (batch,) + src.shape)),
              "per_instance_distinct": np.ascontiguousarray(np.stack([src * (1.0 - 0.5 * k / batch) for k in range(batch)]))}
    h = Handle(flat)
    try:
        info = h.info()
        out_v = torch.empty((batch, st + 1, info["n_out"]), dtype=torch.float64, device=dev)
        out_i = torch.empty((batch, st + 1, info["n_cur"]), dtype=torch.float64, device=dev)
        for name, tab in tables.items():
            d_src = torch.from_numpy(tab).to(dev)
            best = None
            for rep in range(reps + 1):  # (the first run is the warm-up)
                h.reset_state()
                h.run_device(st, dt, d_src.data_ptr(), out_v.data_ptr(), out_i.data_ptr(), src_per_inst=tab.ndim == 3)
                rc = h.sync()
                assert rc == 0, h.error()
                if rep > 0:
                    best = h.kernel_ms() if best is None else min(best, h.kernel_ms())
            print(json.dumps(dict(case="kernel", tables=name, nodes=n, n_inst=batch, points=st + 1, kernel_ms=best,
                                  solves_per_s=h.solves() / (best * 1e-3), interpreter=info["interpreter"],
                                  inst_per_wg=info["inst_per_wg"], threads=info["threads"])), flush=True)
            del d_src
    finally:
        h.close()


def end_to_end(n_var):
    base = golden_netlist(load_golden("boost_probe"))
    texts = [variant(base, k / 16) for k in range(n_var)]  # (values and amplitude scaled by up to 2.1x and 1.8x)
    for exact in (False, True):
        batch = [parseNetlist(t) for t in texts]
        t0 = time.perf_counter()
        got = simulateTRANBatch(batch, exact_order=exact)
        t_batch = time.perf_counter() - t0
        loop = [parseNetlist(t) for t in texts]
        t0 = time.perf_counter()
        ref = [simulateTRAN(c, exact_order=exact) for c in loop]
        t_loop = time.perf_counter() - t0
        same = all(list(a["nodeVoltages"]) == list(b["nodeVoltages"]) for a, b in zip(got, ref))
        print(json.dumps(dict(case="end_to_end", circuit="boost_probe", variants=n_var, mode="exact" if exact else "default",
                              batch_s=t_batch, loop_s=t_loop, speedup=t_loop / t_batch, same_keys=same)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--variants", type=int, default=256)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-end-to-end", action="store_true")
    a = ap.parse_args()
    if not a.skip_kernel:
        kernel_cases(a.nodes, a.batch, a.steps, a.reps)
    if not a.skip_end_to_end:
        end_to_end(a.variants)


if __name__ == "__main__":
    main()
