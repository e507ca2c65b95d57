#!/usr/bin/env python3
"""Sensitivity analysis probe, one JSON line per batch size: on --inst swept instances x --freqs frequencies of an R-C ladder
of --n nodes, one handle that records the output node alone,
  plain_ms / sens_sweeps_ms   AcHandle.run (currents recorded) and the two sweeps of AcHandle.run_sens (spicey_ac_last_kernel_ms:
                their sum), alternating --reps times in one process: every run's kernel time, medians and spreads (max - min)
  sens_ms / sens_full_ms      the reduction pass without and with d_full (spicey_ac_last_sens_ms, HIP events): all runs, medians
  bytes_back / bytes_back_full / bytes_sweeps   what run_sens copies back against out_v + out_i of its two sweeps
  spectrum_bytes / spectrum_bytes_full          what the spectrum kernel must read and write (both rows of currents, H's
                columns, values, tolerances; d_spec and d_full)
and, with --fd-n > 0, on ONE R-C ladder of --fd-n nodes the wall time of the finite-difference route (simulateACBatch of
2 nE + 1 variants, the central differences of the output formed on the host) against simulateSens with full=True, and how far
the two are apart.  --check compares the device's results with reduce_reference_sens on the copied-back sweeps, bit for bit."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spicey_amd import abi, synth  # noqa: E402
from spicey_amd import ac as sac  # noqa: E402
from spicey_amd.ac_batch import simulateACBatch  # noqa: E402
from spicey_amd.lib import AcHandle  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402
from spicey_amd.sens import reduce_reference_sens, simulateSens  # noqa: E402


def stats(xs):
    return {"runs": [round(x, 4) for x in xs], "median": float(np.median(xs)), "spread": float(max(xs) - min(xs))}


def batch(a, freqs, ni):
    flat, _, _, _ = synth.chain_batch("rc_ladder", a.n, range(1, ni + 1), tran=".tran 1e-6 3e-5")
    out = flat.n_nodes
    flat.out_nodes = np.array([out], np.int32)
    nE = flat.nR + flat.nC + flat.nL
    n_cur = nE + flat.nV
    nf = len(freqs)
    tol = np.where(np.arange(nE) < flat.nR, 0.01, 0.05)
    req = abi.ac_sens_req(0, -1, flat.nR, flat.nC, flat.nL)
    one = np.array([1.0 + 0j])
    h = AcHandle(flat)
    plain, sweeps, red, red_full = [], [], [], []
    res = None
    for _ in range(a.reps):  # (alternating: plain, sens, sens with full)
        p = h.run(freqs, one)
        assert p["status"] == 0, p["detail"]
        plain.append(p["kernel_ms"])
        res = h.run_sens(freqs, one, out, 0, req, tol)
        assert res["status"] == 0, res["detail"]
        sweeps.append(res["kernel_ms"])
        red.append(res["sens_ms"])
        resf = h.run_sens(freqs, one, out, 0, req, tol, full=True)
        assert resf["status"] == 0, resf["detail"]
        red_full.append(resf["sens_ms"])
    info = h.info()
    t0 = time.perf_counter()
    h.run_sens(freqs, one, out, 0, req, tol)
    wall = (time.perf_counter() - t0) * 1e3
    slots = ni * nf
    spectrum_bytes = slots * (2 * nE * 16 + 16 + abi.SENS_SPEC * 8) + ni * nE * 8 + nE * 8
    rec = dict(case="sens", n=a.n, inst=ni, freqs=nf, nE=nE, mode="resident sweep" if info["interpreter"] == 2 else "one workgroup per solve",
               plain_ms=stats(plain), sens_sweeps_ms=stats(sweeps), sweeps_over_plain=float(np.median(sweeps) / np.median(plain)),
               sens_ms=stats(red), sens_full_ms=stats(red_full), sens_wall_ms=wall,
               bytes_back=int(res["spec"].nbytes + res["peak"].nbytes), bytes_back_full=int(resf["spec"].nbytes + resf["peak"].nbytes + resf["full"].nbytes),
               bytes_sweeps=int(2 * slots * (1 + n_cur) * 16), spectrum_bytes=int(spectrum_bytes), spectrum_bytes_full=int(spectrum_bytes + slots * nE * 16))
    if a.check:
        d = h.run(freqs, one)
        x = h.run_inject(freqs, None, out, 0)
        ref = reduce_reference_sens(d["out_v"], d["out_i"], x["out_i"], flat.R_val, flat.C_val, flat.L_val, tol, freqs, 0, -1)
        eq = lambda u, v: bool(((u.view(np.int64) == v.view(np.int64)) | (np.isnan(u) & np.isnan(v))).all())  # noqa: E731
        rec["same_bits"] = eq(ref[0], resf["spec"]) and eq(ref[1], resf["peak"]) and eq(ref[2], resf["full"]) and eq(ref[0], res["spec"]) and eq(ref[1], res["peak"])
    h.close()
    print(json.dumps(rec), flush=True)


def finite_differences(a, freqs):
    """One circuit: 2 nE + 1 variants through simulateACBatch and differences on the host, against simulateSens."""
    ckt = parseNetlist(synth.rc_ladder(a.fd_n, 1, tran=".tran 1e-6 3e-5"))
    ckt.V[0].acMag = 1.0  # (the ladder's source is a pulse without an AC part)
    # (simulateACBatch sweeps a circuit's .ac card: the probe's frequency list as a card)
    ckt.analyses = dict(ckt.analyses, ac=dict(mode="dec", N=(len(freqs) - 1) / 5.0, f1=1e3, f2=1e8))
    out = ckt.nodes.rev[ckt.nodes.count() - 1]
    hstep = 1e-3
    t0 = time.perf_counter()
    variants = [ckt]
    for kind in ("R", "C", "L"):  # (the value's attribute has the kind's name)
        for e, el in enumerate(getattr(ckt, kind)):
            for s in (1 + hstep, 1 - hstep):
                c = copy.copy(ckt)
                setattr(c, kind, list(getattr(ckt, kind)))
                getattr(c, kind)[e] = copy.copy(el)
                setattr(getattr(c, kind)[e], kind, getattr(el, kind) * s)
                variants.append(c)
    res = simulateACBatch(variants)
    H = np.array(res[0]["nodeVoltages"][out])
    up = np.array([r["nodeVoltages"][out] for r in res[1::2]])
    dn = np.array([r["nodeVoltages"][out] for r in res[2::2]])
    rel_fd = ((up - dn) / (2 * hstep) / H[None, :]).T
    fd_wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    r = simulateSens(ckt, f"v({out})", freqs=res[0]["freqs"], full=True)
    sens_wall = time.perf_counter() - t0
    names = [e.name for e in ckt.R] + [e.name for e in ckt.C] + [e.name for e in ckt.L]
    rel = np.stack([np.array(r["mag_sens"][n]) + 1j * np.radians(np.array(r["phase_sens_deg"][n])) for n in names], axis=1)
    print(json.dumps(dict(case="fd_route", n=a.fd_n, freqs=len(res[0]["freqs"]), nE=len(names), variants=len(variants), fd_wall_s=fd_wall, sens_wall_s=sens_wall,
                          fd_over_sens=fd_wall / sens_wall, worst_abs_difference=float(np.abs(rel - rel_fd).max()),
                          largest_sensitivity=float(np.abs(rel).max()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--inst", type=int, nargs="*", default=[512])
    ap.add_argument("--freqs", type=int, default=201)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=1)
    ap.add_argument("--fd-n", type=int, default=60)
    a = ap.parse_args()
    freqs = np.array(sac.logspace(1e3, 1e8, (a.freqs - 1) / 5.0))[: a.freqs]
    for ni in a.inst:
        batch(a, freqs, ni)
    if a.fd_n > 0:
        finite_differences(a, freqs)


if __name__ == "__main__":
    main()
