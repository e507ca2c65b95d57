#!/usr/bin/env python3
"""Cost of a corner sweep with and without the batched AC measurements, one JSON line.
  measureACBatch   --variants variants of tests/golden/netlists/ac_readme.cir with three measures (the -3 dB corner, the
                   peak, a point read-out): one handle, one launch, 8 doubles per (circuit, measure) back
  simulateAC loop  the same circuits through simulateAC one by one — one handle, one launch and every node's and element's
                   response copied back per circuit — and the same three numbers from the returned lists by numpy
Wall seconds (parsing excluded), best of --rounds in alternating order after one warm-up round, plus the reduction's own
time (spicey_ac_last_measure_ms, HIP events) of one AcHandle.run_measure on the same batch."""
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
from spicey_amd import abi, lib  # noqa: E402
from spicey_amd import ac as sac  # noqa: E402
from spicey_amd.ac_batch import stacked  # noqa: E402
from spicey_amd.ac_measure import _Plan, at, extrema, fcross, measureACBatch  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    with open(os.path.join(REPO, "tests", "golden", "netlists", "ac_readme.cir")) as f:
        base = f.read()
    texts = [variant(base, k / 16) for k in range(a.variants)]
    m = {"fc": fcross("v(2)/v(1)", 0.5 ** 0.5), "pk": extrema("v(2)"), "lo": at("v(2)", 10.0)}
    t_meas, t_loop = [], []
    for rnd in range(a.rounds + 1):  # (round 0 is the warm-up)
        for which in (("measure", "loop") if rnd % 2 == 0 else ("loop", "measure")):
            ckts = [parseNetlist(t) for t in texts]
            t0 = time.perf_counter()
            if which == "measure":
                got = measureACBatch(ckts, m)
                dt = time.perf_counter() - t0
                if rnd:
                    t_meas.append(dt)
            else:
                ref = []
                for c in ckts:
                    r = sac.simulateAC(c)
                    h = np.asarray(r["nodeVoltages"]["2"]) / np.asarray(r["nodeVoltages"]["1"])
                    q = h.real * h.real + h.imag * h.imag
                    k = int(np.nonzero((q[:-1] > 0.5) & (q[1:] <= 0.5))[0][0])
                    v2 = np.abs(np.asarray(r["nodeVoltages"]["2"]))
                    ref.append((r["freqs"][k], float(v2.max())))
                dt = time.perf_counter() - t0
                if rnd:
                    t_loop.append(dt)
    same = all(g["fc"]["f_lo"] == r[0] and abs(g["pk"]["max"] - r[1]) <= 1e-9 * r[1] for g, r in zip(got, ref))
    # the reduction's own time on the same batch
    ckts = [parseNetlist(t) for t in texts]
    freqs = np.asarray(sac.buildFrequencyArray(**ckts[0].analyses["ac"]))
    plan = _Plan(ckts[0], m, freqs, "dec")
    flat, vph = stacked(ckts, list(range(len(ckts))), plan.flatten)
    h = lib.AcHandle(flat)
    h.run_measure(freqs, vph, plan.reqs)
    res = h.run_measure(freqs, vph, plan.reqs)
    h.close()
    assert res["status"] == abi.OK
    print(json.dumps(dict(case="ac_measure", circuit="ac_readme", variants=a.variants, n_freq=len(freqs), measures=len(m),
                          measureACBatch_s=min(t_meas), simulateAC_loop_s=min(t_loop), ratio=min(t_loop) / min(t_meas),
                          measureACBatch_all_s=t_meas, simulateAC_loop_all_s=t_loop, sweep_kernel_ms=res["kernel_ms"],
                          measure_ms=res["measure_ms"], same_numbers=bool(same))), flush=True)


if __name__ == "__main__":
    main()
