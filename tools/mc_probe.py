#!/usr/bin/env python3
"""Monte Carlo tolerance analysis probe, JSON lines: on --inst samples x --freqs frequencies of the R-C ladder of --n nodes, one
handle that records the output node alone,
  plain_ms / mc_sweep_ms   AcHandle.run without currents and the sweep of AcHandle.run_mc (spicey_ac_last_kernel_ms), alternating
                --reps times in one process: every run's kernel time, medians and spreads (max - min)
  draw_ms / reduce_ms      the draw's and the reduction's event times (spicey_ac_last_mc_draw_ms, spicey_ac_last_mc_ms)
  bytes_back / bytes_sweep what run_mc copies back against out_v + out_i of a sweep that returns everything
and, with --host-inst > 0, the wall time of simulateMonteCarlo against the host route — simulateACBatch of the mc_values variants,
np.sort and the same interpolation on the host — on the same ladder at --host-inst samples, alternating --host-reps times, and how
far the two are apart.  --check compares the device's results with reduce_reference_mc on the plain sweep of a second handle whose
rows are draw_reference_mc's values, bit for bit."""
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
from spicey_amd.mc import icdf_table, mc_gains, mc_ranks, mc_values, quantile_curves, reduce_reference_mc, simulateMonteCarlo  # noqa: E402
from spicey_amd.netlist import parseNetlist  # noqa: E402

PROBS = (0.01, 0.5, 0.99)


def stats(xs):
    return {"runs": [round(x, 4) for x in xs], "median": float(np.median(xs)), "spread": float(max(xs) - min(xs))}


def ladder(n):
    ckt = parseNetlist(synth.rc_ladder(n, 1, tran=".tran 1e-6 3e-5"))
    ckt.V[0].acMag = 1.0  # (the ladder's source is a pulse without an AC part)
    return ckt


def batch(a, freqs, ni):
    ckt = ladder(a.n)
    flat = abi.flatten(ckt)
    out = flat.n_nodes
    flat.out_nodes = np.array([out], np.int32)
    flat = flat.replicate(ni)
    nE = flat.nR + flat.nC + flat.nL
    nf = len(freqs)
    tol = np.where(np.arange(nE) < flat.nR, 0.01, 0.05)
    icdf, log2K = icdf_table("gauss")
    req = abi.ac_mc_req(0, -1, log2K, True, a.seed)
    lo = np.full(nf, 0.0)
    one = np.array([1.0 + 0j])
    h = AcHandle(flat)
    plain, sweep, draw, red = [], [], [], []
    res = None
    for _ in range(a.reps):  # (alternating: plain, mc)
        p = h.run(freqs, one, want_currents=False)
        assert p["status"] == 0, p["detail"]
        plain.append(p["kernel_ms"])
        res = h.run_mc(freqs, one, req, tol, icdf, lo, None, PROBS)
        assert res["status"] == 0, res["detail"]
        sweep.append(res["kernel_ms"])
        draw.append(res["draw_ms"])
        red.append(res["mc_ms"])
    info = h.info()
    t0 = time.perf_counter()
    h.run_mc(freqs, one, req, tol, icdf, lo, None, PROBS)
    wall = (time.perf_counter() - t0) * 1e3
    h.close()
    slots = ni * nf
    rec = dict(case="mc", n=a.n, inst=ni, freqs=nf, nE=nE, mode="resident sweep" if info["interpreter"] == 2 else "one workgroup per solve",
               plain_ms=stats(plain), mc_sweep_ms=stats(sweep), sweep_over_plain=float(np.median(sweep) / np.median(plain)), draw_ms=stats(draw),
               reduce_ms=stats(red), mc_wall_ms=wall, bytes_back=int(res["freq_stats"].nbytes + res["sample"].nbytes + res["nominal"].nbytes),
               bytes_sweep=int(slots * (1 + nE + flat.nV) * 16), bytes_sweep_all_nodes=int(slots * (flat.n_nodes + nE + flat.nV) * 16),
               bytes_keys=int(nf * (1 << (ni - 1).bit_length()) * 8))
    if a.check:
        g = mc_gains(ni, tol, icdf, log2K, a.seed, True)
        drawn = flat.replicate(ni)
        drawn.R_val = np.ascontiguousarray(flat.R_val * g[:, :flat.nR])
        drawn.C_val = np.ascontiguousarray(flat.C_val * g[:, flat.nR:flat.nR + flat.nC])
        h2 = AcHandle(drawn)
        d = h2.run(freqs, one, want_currents=False)
        h2.close()
        rs, rf = reduce_reference_mc(d["out_v"], 0, -1, None, lo, None, mc_ranks(PROBS, ni))
        eq = lambda u, v: bool(((u.view(np.int64) == v.view(np.int64)) | (np.isnan(u) & np.isnan(v))).all())  # noqa: E731
        rec["same_bits"] = eq(rf, res["freq_stats"]) and bool((rs == res["sample"]).all())
    print(json.dumps(rec), flush=True)


def host_route(a, freqs):
    """simulateMonteCarlo against simulateACBatch of the mc_values variants with np.sort on the host."""
    ckt = ladder(a.n)
    # (simulateACBatch sweeps a circuit's .ac card: the probe's frequency list as a card)
    ckt.analyses = dict(ckt.analyses, ac=dict(mode="dec", N=(len(freqs) - 1) / 5.0, f1=1e3, f2=1e8))
    out = ckt.nodes.rev[ckt.nodes.count() - 1]
    tol = {"R": 0.01, "C": 0.05}
    n = a.host_inst
    host, dev, worst = [], [], 0.0
    for _ in range(a.host_reps):  # (alternating)
        t0 = time.perf_counter()
        variants = []
        for s in range(n):
            vals = mc_values(ckt, tol, a.seed, s)
            c = copy.copy(ckt)
            c.R = [copy.copy(e) for e in ckt.R]
            c.C = [copy.copy(e) for e in ckt.C]
            for e in c.R:
                e.R = vals[e.name]
            for e in c.C:
                e.C = vals[e.name]
            variants.append(c)
        res = simulateACBatch(variants)
        H = np.array([r["nodeVoltages"][out] for r in res])
        q = np.sort(H.real * H.real + H.imag * H.imag, axis=0)
        st = np.zeros((q.shape[1], abi.MC_FREQ_HEAD + 2 * len(PROBS)))
        st[:, abi.MC_FREQ_HEAD:] = q[mc_ranks(PROBS, n)].T
        curves = quantile_curves(st, PROBS, n)
        host.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        r = simulateMonteCarlo(ckt, f"v({out})", tol=tol, n=n, seed=a.seed, quantiles=PROBS)
        dev.append(time.perf_counter() - t0)
        # (relative to the host's curve; where the ladder's response underflows to 0 both are 0)
        worst = max(worst, max(float((np.abs(np.array(r["mag"][p]) - c) / np.maximum(c, 1e-300)).max()) for p, c in zip(PROBS, curves)))
    print(json.dumps(dict(case="host_route", n=a.n, inst=n, freqs=len(freqs), host_wall_s=stats(host), mc_wall_s=stats(dev),
                          host_over_mc=float(np.median(host) / np.median(dev)), worst_relative_difference=worst,
                          bytes_host_route=int(n * len(freqs) * (ckt.nodes.count() - 1 + len(ckt.R) + len(ckt.C) + len(ckt.V)) * 16))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--inst", type=int, nargs="*", default=[4096])
    ap.add_argument("--freqs", type=int, default=201)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--check", type=int, default=1)
    ap.add_argument("--host-inst", type=int, default=256)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    freqs = np.array(sac.logspace(1e3, 1e8, (a.freqs - 1) / 5.0))[: a.freqs]
    for ni in a.inst:
        batch(a, freqs, ni)
    if a.host_inst > 0:
        host_route(a, freqs)


if __name__ == "__main__":
    main()
