#!/usr/bin/env python3
"""Periodic-steady-state probe, JSON lines.  Per fixture (--circuits, of tests/pss_cases.py) and circuit count (--n-ckt), one handle
of n_ckt (1 + nX) instances, --reps times in one process:
  newton    Handle.run_pss with method newton: iterations, wall ms of the call, and by events the designs plus updates (pss_ms)
            and the transients' kernels (tran_ms), each summed over the iterations and per iteration
  settle    a second handle of n_ckt instances, method settle, max_iter --settle-max: periods until the same stopping rule, wall ms,
            and the same two event sums
and, with --update-nx N > 0, the update alone at nX = N on --update-ckt seeded contracting maps (tests/pss_host/pypss.py
linear_case): event ms of spicey_pss_update_device over --reps launches, checked against the numpy restatement bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import pss_cases as pc  # noqa: E402
from spicey_amd import abi, pss  # noqa: E402
from spicey_amd.lib import Handle  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402


def spread(xs):
    return {"runs": [round(float(x), 4) for x in xs], "median": float(np.median(xs)), "spread": float(max(xs) - min(xs))}


def run_case(name, n_ckt, a):
    ckt = parseNetlist(pc.NETLISTS[name])
    dt, _ = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    m = pc.STEPS_PER_PERIOD[name]
    src = pss.period_table(ckt, dt, m)
    one = abi.flatten(ckt)
    one.out_nodes = np.array([1], np.int32)
    nX = one.nC + one.nL + one.nD
    out = {"probe": "pss", "circuit": name, "n_ckt": n_ckt, "nX": nX, "steps_per_period": m}
    for method, W, max_iter in (("newton", 1 + nX, a.max_iter), ("settle", 1, a.settle_max)):
        flat = one.replicate(n_ckt * W)
        req = abi.pss_req(n_ckt, abi.PSS_METHODS[method], max_iter)
        wall, pss_ms, tran_ms, iters, res = [], [], [], None, None
        for _ in range(a.reps):
            h = Handle(flat)
            try:
                t0 = time.perf_counter()
                r = h.run_pss(m, dt, src, req)
                wall.append((time.perf_counter() - t0) * 1e3)
            finally:
                h.close()
            assert r["status"] == abi.OK, r["detail"]
            pss_ms.append(r["pss_ms"])
            tran_ms.append(r["tran_ms"])
            iters, res = int(r["n_iter"].max()), float(r["history"][-1][:, 0].max())
            status = sorted(set(int(s) for s in r["ckt_status"]))
        out[method] = {"instances": n_ckt * W, "iterations": iters, "periods_simulated_per_circuit": iters * W, "status": status, "last_res": res,
                       "wall_ms": spread(wall), "design_update_ms": spread(pss_ms), "transient_ms": spread(tran_ms),
                       "design_update_ms_per_iteration": float(np.median(pss_ms)) / iters, "transient_ms_per_iteration": float(np.median(tran_ms)) / iters}
    return out


def update_alone(a):
    import torch

    from pss_host import pypss as pp
    from spicey_amd import lib
    nX, n_ckt = a.update_nx, a.update_ckt
    kinds, req, base, base_on, h, X, on, done, _ = pp.linear_case(nX, n_ckt, seed=5)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    parts = [dev(p) if p.size else None for p in pp.split(X, kinds)]
    d_h, d_on = dev(h), dev(on)
    d_delta = torch.zeros((n_ckt, nX), dtype=torch.float64, device="cuda")
    d_rows = torch.zeros((n_ckt, abi.PSS_ROW), dtype=torch.float64, device="cuda")
    need = lib.pss_workspace_bytes(n_ckt, nX)
    d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
    ms = []
    for _ in range(a.reps + 1):  # (the first launch raises the kernel's dynamic-LDS limit and loads the code object)
        d_base, d_bon, d_done = dev(base), dev(base_on), dev(done)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        lib.pss_update_device(kinds, base_on.shape[1], req, None, ptr(d_base), ptr(d_bon), ptr(d_h), *(ptr(p) for p in parts), ptr(d_on), ptr(d_delta), ptr(d_rows),
                              ptr(d_done), d_work.data_ptr(), need, stream=torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ref = pp.reference_update(kinds, req, base, base_on, h, X, on, done)
    same = bool((d_base.cpu().numpy().view(np.int64) == ref[0].view(np.int64)).all() and (d_rows.cpu().numpy().view(np.int64) == ref[3].view(np.int64)).all())
    return {"probe": "pss_update", "nX": nX, "n_ckt": n_ckt, "lds_bytes": nX * (nX + 1) * 8, "first_launch_ms": ms[0], "update_ms": spread(ms[1:]), "bits_equal_numpy": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuits", default="PSS_BUCK,PSS_BOOST_SLOW")
    ap.add_argument("--n-ckt", default="1,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--settle-max", type=int, default=1000)
    ap.add_argument("--update-nx", type=int, default=128)
    ap.add_argument("--update-ckt", type=int, default=1)
    a = ap.parse_args()
    if a.update_nx > 0:  # (torch opens the device before the library does: spicey_amd/lib.py load())
        print(json.dumps(update_alone(a)), flush=True)
    for name in [c for c in a.circuits.split(",") if c]:
        for n_ckt in [int(v) for v in a.n_ckt.split(",")]:
            print(json.dumps(run_case(name, n_ckt, a)), flush=True)


if __name__ == "__main__":
    main()
