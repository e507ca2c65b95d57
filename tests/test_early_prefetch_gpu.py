"""Early-prefetch kernels (tran_v2_run.h: EP — Z's element parameters from one record per thread, fetched with the next source
value under the tridiagonal top) on the GPU against the same shape's plain kernels: every case runs with
SPICEY_NO_EARLY_PREFETCH set and without it and must give the same bits — voltages, currents, iteration counts, end state —
and the run without the knob is held against the oracle at the project's bar.  33 steps unless a case says otherwise."""
from __future__ import annotations

import numpy as np
import pytest

from batch_variants import instance
from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist
from test_gpu_parity import tol_ratio
from test_packed_resident_gpu import _switched_ladder

pytestmark = pytest.mark.gpu

STEPS = 33
KNOB = "SPICEY_NO_EARLY_PREFETCH"


def _chain(kind, n, seeds=(1, 2), steps=STEPS):
    flat, dt, total, src = synth.chain_batch(kind, n, list(seeds), tran=".tran 1e-6 4e-5")
    assert total >= steps
    return flat, dt, src[: steps + 1], steps


def _mesh34():
    ckt = parseNetlist(synth.rcd_mesh(34, tran=".tran 1e-6 4e-5"))
    dt, total = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt)
    assert flat.nR > 2 * 512 and total >= STEPS  # beyond the two resident items of 512 threads
    return flat.replicate(2), dt, abi.source_table(ckt, dt, total)[: STEPS + 1], STEPS


def _switched():
    flat, dt, src = _switched_ladder()
    return flat, dt, src[: STEPS + 1], STEPS


def _three_sources(n=300):
    """A diode chain fed at both ends and in the middle by three different pulses: three values per step to fetch and park."""
    L = ["* chain with three sources", ".model DM D(Is=1e-14 N=1)",
         "V1 n1 0 PULSE(0 5 0 1e-6 1e-6 4e-6 1e-5)", f"V2 m 0 PULSE(0 3 2e-6 1e-6 1e-6 3e-6 8e-6)", f"V3 n{n} 0 PULSE(1 4 1e-6 2e-6 1e-6 5e-6 1.2e-5)",
         f"RM m n{n // 2} 50"]
    for k in range(1, n):
        L.append(f"R{k} n{k} n{k+1} {100 * (1 + 0.001 * (k % 17)):.6g}")
        L.append(f"C{k} n{k+1} 0 {1e-9 * (1 + 0.002 * (k % 11)):.6g}")
        if k % 2: L.append(f"D{k} n{k+1} 0 DM")
    L += [".tran 1e-6 4e-5", ".end", ""]
    ckt = parseNetlist("\n".join(L))
    dt, total = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt).replicate(2)
    flat.R_val[1] *= 1.03
    assert flat.nV == 3 and total >= STEPS
    return flat, dt, abi.source_table(ckt, dt, total)[: STEPS + 1], STEPS


# name: (circuit, geometry, the plan must take the packed fresh shape — the one with early-prefetch kernels)
CASES = {
    "diode_chain_1000": (lambda: _chain("diode_chain", 1000), 2, True),   # the bench build, two instances
    "diode_chain_100": (lambda: _chain("diode_chain", 100), 2, True),     # most threads own no item: zero-filled record slots
    "diode_chain_333": (lambda: _chain("diode_chain", 333), 2, True),     # element counts that are no multiple of a wave or of the workgroup
    "rcd_mesh_34": (_mesh34, 0, False),                                   # > 2 x 512 resistors: the beyond-resident loops, whichever build the plan gives
    "switched_ladder": (_switched, 2, True),                              # nS > 0: B runs again within a step
    "three_sources": (_three_sources, 2, True),
    "one_step": (lambda: _chain("diode_chain", 100, steps=1), 2, True),   # the first fetch is also the last: nothing past the end of the source table
    "two_steps": (lambda: _chain("diode_chain", 100, steps=2), 2, True),
    "rc_ladder_100": (lambda: _chain("rc_ladder", 100), 0, False),        # linear: factor reuse, the default program
}


def _run(flat, dt, src, steps, geometry, runs=1):
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=geometry)
    try:
        out = []
        for _ in range(runs):
            r = h.run(steps, dt, src)
            assert r["status"] == 0, r["detail"]
            out.append(r)
        return out, h.info()
    finally:
        h.close()


def _same_bits(a, b, what):
    for k in ("out_v", "out_i"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    assert np.array_equal(a["iters"], b["iters"]), (what, "iters")
    for k, v in a["state"].items():
        assert np.array_equal(np.asarray(v), np.asarray(b["state"][k]), equal_nan=(k != "S_ison")), (what, "state", k)


def _both(monkeypatch, flat, dt, src, steps, geometry, runs=1):
    monkeypatch.setenv(KNOB, "1")
    off, info_off = _run(flat, dt, src, steps, geometry, runs)
    monkeypatch.delenv(KNOB)
    on, info_on = _run(flat, dt, src, steps, geometry, runs)
    assert info_on == info_off  # the same plan: the knob picks between two kernels of one shape
    return off, on, info_on


def _against_oracle(oracle_backend, got, one, j, steps, dt, src, switches):
    ref = oracle_backend.run(one, steps, dt, src)
    assert ref["status"] == 0
    assert tol_ratio(got["out_v"][j], ref["out_v"][0]).max() <= 1.0 and tol_ratio(got["out_i"][j], ref["out_i"][0]).max() <= 1.0
    if switches:
        assert np.array_equal(got["iters"][j], ref["iters"][0])
    return ref


@pytest.mark.parametrize("case", sorted(CASES))
def test_knob_off_and_on_give_the_same_bits_and_the_oracles_values(case, oracle_backend, monkeypatch):
    make, geometry, packed_fresh = CASES[case]
    flat, dt, src, steps = make()
    off, on, info = _both(monkeypatch, flat, dt, src, steps, geometry)
    if packed_fresh:
        assert info["geometry"] == 2 and info["threads"] == 512 and info["resident_slots"] == 4
    _same_bits(off[0], on[0], case)
    if case == "switched_ladder":
        assert flat.nS > 0 and int(on[0]["iters"].max()) > 1
    j = flat.n_inst - 1
    _against_oracle(oracle_backend, on[0], instance(flat, j), j, steps, dt, src, flat.nS > 0)


def test_two_runs_on_one_handle(oracle_backend, monkeypatch):
    """The second run starts from the first one's end state and from a record that its own prologue rebuilt."""
    flat, dt, src, steps = _chain("diode_chain", 333)
    off, on, _ = _both(monkeypatch, flat, dt, src, steps, 2, runs=2)
    for r in (0, 1):
        _same_bits(off[r], on[r], f"run {r}")
    assert not np.array_equal(on[0]["out_v"], on[1]["out_v"])  # (the state did carry over)
    j = 1
    ref0 = _against_oracle(oracle_backend, on[0], instance(flat, j), j, steps, dt, src, False)
    nxt = instance(flat, j)
    for k in ("C_vprev", "L_iprev", "D_vdprev"):
        setattr(nxt, k, np.array(ref0["state"][k], dtype=np.float64).reshape(getattr(nxt, k).shape))
    _against_oracle(oracle_backend, on[1], nxt, j, steps, dt, src, False)
