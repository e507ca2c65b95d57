#!/usr/bin/env python3
"""Throughput of the reference-order engine (SpiceyOptions.interpreter = 3) next to the default sparse path on the same
inputs: solves/s and us per step of the kernel (HIP events, spicey_last_kernel_ms), one JSON line per (case, engine).
  dchain20, mesh9x5            the goldens, one instance each
  diode_chain(20) x 512        512 distinct instances (values from seeds 0..511), one launch
  diode_chain(1000)            one instance, global slab in exact mode (200 steps)"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import golden_netlist, load_golden  # noqa: E402
from spicey_amd import abi, synth  # noqa: E402
from spicey_amd.lib import Handle  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402


def setup(text):
    ckt = parseNetlist(text)
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    return abi.flatten(ckt), steps, dt, abi.source_table(ckt, dt, steps)


def measure(name, flat, steps, dt, src, interpreter, reps=3):
    h = Handle(flat, interpreter=interpreter)
    try:
        info = h.info()
        r = h.run(steps, dt, src)  # (warm-up; continues the transient afterwards, which changes no cost)
        assert r["status"] == 0, r["detail"]
        best = None
        for _ in range(reps):
            r = h.run(steps, dt, src)
            best = r["kernel_ms"] if best is None else min(best, r["kernel_ms"])
        solves = r["solves"]
    finally:
        h.close()
    print(json.dumps(dict(case=name, engine="exact" if interpreter == 3 else "default", n_var=flat.n_var, n_inst=flat.n_inst, points=steps + 1,
                          solves=solves, kernel_ms=best, solves_per_s=solves / (best * 1e-3), us_per_step=best * 1e3 / (steps + 1),
                          threads=info["threads"], lds_bytes=info["lds_bytes"])), flush=True)


def main():
    cases = [("dchain20", setup(golden_netlist(load_golden("dchain20")))), ("mesh9x5", setup(golden_netlist(load_golden("mesh9x5"))))]
    flats = [setup(synth.diode_chain(20, seed=s, tran=".tran 1e-6 1e-4")) for s in range(512)]
    cases.append(("diode_chain(20) x 512", (abi.stack_instances([f[0] for f in flats]),) + flats[0][1:]))
    cases.append(("diode_chain(1000)", setup(synth.diode_chain(1000, seed=2, tran=".tran 1e-6 2e-4"))))
    for name, (flat, steps, dt, src) in cases:
        for interp in (3, 0):
            measure(name, flat, steps, dt, src, interp, reps=1 if flat.n_var > 500 else 3)


if __name__ == "__main__":
    main()
