#!/usr/bin/env python3
"""Noise analysis probe, one JSON line per batch size: on --inst swept instances x --freqs frequencies of an R-C ladder of
--n nodes
  plain_ms      the un-injected sweep (AcHandle.run), best kernel time of --reps
  inject_ms     the same sweep with a unit current injected at the last node (AcHandle.run_inject)
  noise_sweep_ms / noise_ms   AcHandle.run_noise: its injected sweep (only the output node recorded) and its reduction pass
                (spicey_ac_last_noise_ms, HIP events)
  bytes_back / bytes_sweep    what run_noise copies back (spec, contrib, total, gain) against the whole sweep's out_v + out_i
  noise_wall_ms / inject_wall_ms   wall time of the calls (allocation, copies back)
and a check of the reduction against reduce_reference_noise on the copied-back sweep (bit for bit)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spicey_amd import abi, synth  # noqa: E402
from spicey_amd import ac as sac  # noqa: E402
from spicey_amd.lib import AcHandle  # noqa: E402
from spicey_amd.noise import kt4_of, reduce_reference_noise  # noqa: E402


def best(call, reps, key="kernel_ms"):
    ms, wall, res = None, None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        w = (time.perf_counter() - t0) * 1e3
        assert res["status"] == 0, res["detail"]
        ms = res[key] if ms is None else min(ms, res[key])
        wall = w if wall is None else min(wall, w)
    return ms, wall, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--inst", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--freqs", type=int, default=201)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=1)
    a = ap.parse_args()
    freqs = np.array(sac.logspace(1e3, 1e8, (a.freqs - 1) / 5.0))[: a.freqs]
    one = np.array([1.0 + 0j])
    for ni in a.inst:
        flat, _, _, _ = synth.chain_batch("rc_ladder", a.n, range(1, ni + 1), tran=".tran 1e-6 3e-5")
        out = flat.n_nodes
        h = AcHandle(flat)
        plain_ms, plain_wall, _ = best(lambda: h.run(freqs, one), a.reps)
        inj_ms, inj_wall, sw = best(lambda: h.run_inject(freqs, None, out, 0), a.reps)
        info = h.info()
        h.close()
        # the noise call records the output node alone
        flat.out_nodes = np.array([out], np.int32)
        in_col = flat.nR + flat.nC + flat.nL
        req = abi.ac_noise_req(0, -1, in_col, kt4_of(300.15))
        h = AcHandle(flat)
        noise_ms, noise_wall, res = best(lambda: h.run_noise(freqs, out, 0, req), a.reps, key="noise_ms")
        sweep_ms = res["kernel_ms"]
        h.close()
        rec = dict(case="noise", n=a.n, inst=ni, freqs=len(freqs), nR=flat.nR, mode="resident sweep" if info["interpreter"] == 2 else "one workgroup per solve",
                   plain_ms=plain_ms, inject_ms=inj_ms, inject_over_plain=inj_ms / plain_ms, noise_sweep_ms=sweep_ms, noise_ms=noise_ms,
                   plain_wall_ms=plain_wall, inject_wall_ms=inj_wall, noise_wall_ms=noise_wall,
                   bytes_back=int(res["spec"].nbytes + res["contrib"].nbytes + res["total"].nbytes + res["gain"].nbytes),
                   bytes_sweep=int(sw["out_v"].nbytes + sw["out_i"].nbytes))
        if a.check:
            spec, contrib, total = reduce_reference_noise(sw["out_v"][:, :, out - 1:out], sw["out_i"], flat.R_val, freqs, req.kt4, 0, -1, in_col)
            eq = lambda x, y: bool(((x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y))).all())  # noqa: E731
            rec["same_bits"] = eq(spec, res["spec"]) and eq(contrib, res["contrib"]) and eq(total, res["total"])
            rec["total_rms_inst0"] = float(np.sqrt(res["total"][0, 0]))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
