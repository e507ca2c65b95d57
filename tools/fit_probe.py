#!/usr/bin/env python3
"""Element-sizing probe, JSON lines.  Per problem (--problems: rc, the two-resistor RC problem of tests/test_fit_run_gpu.py, and the
fixtures of tests/pss_cases.py named in --circuits, sized on their first inductor and capacitor towards a ripple and an average
taken from the nominal run) and number of starts (--starts), --reps times in one process:
  device    optimizeTRAN through spicey_run_fit: iterations, wall ms of the call, and by events the designs plus updates (fit_ms)
            and the transients' kernels (kernel_ms), each summed over the iterations; the bytes brought back per iteration
  host      the same call through host_run_fit on the same backend: wall ms, and whether its history equals the device's bit for bit
and, with --update-na N > 0, the update alone at nA = N on --update-ckt seeded problems of --update-scalars goals
(tests/fit_host/pyfit.py random_case): event ms of spicey_fit_update_device over --reps launches, checked against numpy bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from spicey_amd import abi, fit, optimizeTRAN  # noqa: E402
from spicey_amd.fit import at_most, target  # noqa: E402
from spicey_amd.measure import measureTRAN, stats  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402

RC = "V1 in 0 5\nR1 in out 1000\nC1 out 0 2e-9\nR2 out 0 2000\n.tran 4e-7 4e-5\n.end\n"


def spread(xs):
    return {"runs": [round(float(x), 4) for x in xs], "median": float(np.median(xs)), "spread": float(max(xs) - min(xs))}


class HostLoop:
    """A backend without run_fit: optimizeTRAN drives it through host_run_fit."""

    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        if name == "run_fit":
            raise AttributeError(name)
        return getattr(self._be, name)


def problem(name):
    """(netlist text, measures, goals, vars) of a named problem."""
    from spicey_amd.lib import HipBackend
    if name == "rc":
        return RC, {"o": stats("v(out)")}, {"o.final": target(3.0, scale=0.01), "o.avg": at_most(2.95, scale=0.01)}, {"R1": (200.0, 5000.0), "R2": (500.0, 8000.0)}
    import pss_cases as pc
    text = pc.NETLISTS[name]
    ckt = parseNetlist(text)
    node = "v(%s)" % ckt.nodes.rev[ckt.C[-1].n1]   # the last capacitor's node: the output of the fixtures
    tran = ckt.analyses["tran"]
    measures = {"o": stats(node, t_from=0.5 * tran["tstop"])}
    nom = measureTRAN(parseNetlist(text), measures, backend=HipBackend())["o"]
    # ask for 0.8 of the nominal ripple at 1.02 of the nominal average, with the first L and C free by a factor of 4
    goals = {"o.pp": at_most(0.8 * nom["pp"], scale=0.01 * nom["pp"]), "o.avg": target(1.02 * nom["avg"], scale=0.001 * abs(nom["avg"]))}
    vars_ = {e.name: (v / 4.0, v * 4.0) for e, v in ((ckt.L[0], ckt.L[0].L), (ckt.C[0], ckt.C[0].C))}
    return text, measures, goals, vars_


def run_problem(name, starts, a):
    from spicey_amd.lib import HipBackend
    text, measures, goals, vars_ = problem(name)
    out = {"probe": "fit", "problem": name, "starts": starts, "nA": len(vars_), "instances": starts * (1 + 2 * len(vars_)), "goals": len(goals)}
    res = {}
    for label, make in (("device", HipBackend), ("host", lambda: HostLoop(HipBackend()))):
        wall, fit_ms, tran_ms = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = optimizeTRAN(parseNetlist(text), measures, goals, vars_, starts=starts, seed=1, max_iter=a.max_iter, backend=make())
            wall.append((time.perf_counter() - t0) * 1e3)
            fit_ms.append(r["fit_ms"] or 0.0)
            tran_ms.append(r["kernel_ms"] or 0.0)
        res[label] = r
        its = max(s["iterations"] for s in r["starts"])
        out[label] = {"iterations": its, "status": [s["status"] for s in r["starts"]], "best_cost": r["cost"], "wall_ms": spread(wall)}
        if label == "device":
            out[label].update(design_update_ms=spread(fit_ms), transient_ms=spread(tran_ms), design_update_ms_per_iteration=float(np.median(fit_ms)) / its,
                              transient_ms_per_iteration=float(np.median(tran_ms)) / its,
                              bytes_back_per_iteration=starts * (abi.FIT_ROW * 8 + 4 + len(goals) * 8),
                              bytes_back_per_iteration_measure_sens=starts * (len(goals) * len(vars_) * (2 * 8 + 1) + len(goals) * 8 * 8 + (1 + 2 * len(vars_)) * len(goals) * 8))
    out["host_over_device_wall"] = out["host"]["wall_ms"]["median"] / out["device"]["wall_ms"]["median"]
    out["histories_bit_equal"] = all(np.array_equal(np.array([list(h.values()) for h in d["history"]]).view(np.int64),
                                                    np.array([list(h.values()) for h in s["history"]]).view(np.int64))
                                     for d, s in zip(res["device"]["starts"], res["host"]["starts"]))
    return out


def update_alone(a):
    import torch

    from fit_host import pyfit as pf
    from spicey_amd import lib
    nA, n_ckt, ns = a.update_na, a.update_ckt, a.update_scalars
    req, step, g_lo, g_hi, goals, x, g, done = pf.random_case(nA, ns, n_ckt, seed=5)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    d_x = dev(x)
    need = lib.fit_workspace_bytes(n_ckt, nA, ns)
    ms = []
    for _ in range(a.reps + 1):  # (the first launch raises the kernel's dynamic-LDS limit and loads the code object)
        d_g, d_done = dev(g), dev(done)
        d_rows = torch.zeros((n_ckt, abi.FIT_ROW), dtype=torch.float64, device="cuda")
        d_work = torch.zeros(need, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        lib.fit_update_device(req, ns, True, step, g_lo, g_hi, goals, None, d_x.data_ptr(), d_g.data_ptr(), d_rows.data_ptr(), d_done.data_ptr(), d_work.data_ptr(), need,
                              stream=torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ref = fit.reduce_reference_fit(req, True, step, g_lo, g_hi, goals, None, x, g, done)
    same = bool((d_g.cpu().numpy().view(np.int64) == ref[0].view(np.int64)).all() and (d_rows.cpu().numpy().view(np.int64) == ref[1].view(np.int64)).all())
    return {"probe": "fit_update", "nA": nA, "n_ckt": n_ckt, "n_scalar": ns, "lds_bytes": nA * (nA + 1) * 8, "first_launch_ms": ms[0], "update_ms": spread(ms[1:]),
            "bits_equal_numpy": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="rc,PSS_BUCK")
    ap.add_argument("--starts", default="1,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--update-na", type=int, default=128)
    ap.add_argument("--update-ckt", type=int, default=1)
    ap.add_argument("--update-scalars", type=int, default=8)
    a = ap.parse_args()
    if a.update_na > 0:  # (torch opens the device before the library does: spicey_amd/lib.py load())
        print(json.dumps(update_alone(a)), flush=True)
    for name in [c for c in a.problems.split(",") if c]:
        for starts in [int(v) for v in a.starts.split(",")]:
            print(json.dumps(run_problem(name, starts, a)), flush=True)


if __name__ == "__main__":
    main()
