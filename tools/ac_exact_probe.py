#!/usr/bin/env python3
"""Kernel time of the reference-order AC engine (spicey_ac_create with SpiceyOptions.interpreter = 3) next to the default
sparse AC path on the same inputs: milliseconds of the sweep's kernels (HIP events, spicey_ac_last_kernel_ms), best of
three runs, one JSON line per (case, engine).
  ac_readme x 201 frequencies     the golden's frequency list, one instance
  ac_ladder30 x 64 instances      perturbed copies in one launch, the golden's 51 frequencies
  ac_mesh6                        the golden's frequencies, one instance
  ac_rc1000 x 16 frequencies      1001 unknowns: the global slab in exact mode"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_golden  # noqa: E402
from spicey_amd import abi  # noqa: E402
from spicey_amd.lib import AcHandle  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402
from test_oracle_ac import ac_golden_netlist, cplx  # noqa: E402


def measure(name, flat, freqs, vph, interpreter, reps=3):
    h = AcHandle(flat, interpreter=interpreter)
    try:
        r = h.run(freqs, vph)  # (warm-up)
        assert r["status"] == 0, r["detail"]
        best = None
        for _ in range(reps):
            r = h.run(freqs, vph)
            best = r["kernel_ms"] if best is None else min(best, r["kernel_ms"])
        info = h.info()
    finally:
        h.close()
    slots = flat.n_inst * len(freqs)
    print(json.dumps(dict(case=name, engine="exact" if interpreter == 3 else "default", n_var=flat.n_var, n_inst=flat.n_inst, n_freq=len(freqs),
                          kernel_ms=best, solves_per_s=slots / (best * 1e-3), threads=info["threads"], lds_bytes=info["lds_bytes"])), flush=True)


def golden_case(name):
    g = load_golden(name)
    return abi.flatten(parseNetlist(ac_golden_netlist(g))), np.array(g["freqs"]), cplx(g["vph"])


def main():
    cases = [("ac_readme x 201", golden_case("ac_readme"))]
    flat, freqs, vph = golden_case("ac_ladder30")
    flats = []
    for k in range(64):
        f = abi.flatten(parseNetlist(ac_golden_netlist(load_golden("ac_ladder30"))))
        f.R_val = f.R_val * (1 + 0.01 * k)
        f.C_val = f.C_val * (1 - 0.005 * k)
        flats.append(f)
    cases.append(("ac_ladder30 x 64", (abi.stack_instances(flats), freqs, vph)))
    cases.append(("ac_mesh6", golden_case("ac_mesh6")))
    cases.append(("ac_rc1000 x 16", golden_case("ac_rc1000")))
    for name, (flat, freqs, vph) in cases:
        for interp in (3, 0):
            measure(name, flat, freqs, vph, interp)


if __name__ == "__main__":
    main()
