"""Packed geometry (two 512-thread workgroups per CU, four resident record slots per thread) with the resident packing that
leaves as few phases streamed as possible: the same bits as the latency geometry, where every record is resident, and the
oracle's values at the project's bar — with the phase table and without it (SPICEY_NO_PHASE_TABLE)."""
from __future__ import annotations

import random

import numpy as np
import pytest

from batch_variants import instance
from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist
from test_gpu_parity import tol_ratio

pytestmark = pytest.mark.gpu

STEPS = 64


def _chain(kind, n):
    flat, dt, steps, src = synth.chain_batch(kind, n, [1, 2, 3, 4], tran=".tran 1e-6 7e-5")
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


def _switched_ladder(n=1000):
    """The ladder of tools/fuzz_switched_ladder.py (series switches on a pulsed control, shunt diodes), one fixed draw."""
    rng = random.Random(3)
    L = ["* switched ladder", ".model SW SW(Ron=1 Roff=1e6 Vt=2.5 Vh=0.2)", ".model DM D(Is=1e-14 N=1)",
         "V1 n1 0 PULSE(0 5 0 1e-6 1e-6 4e-6 1e-5)", "VC ctl 0 PULSE(0 5 2e-6 1e-6 1e-6 3e-6 8e-6)"]
    for k in range(1, n):
        if k % rng.choice([37, 50, 97]) == 0: L.append(f"S{k} n{k} n{k+1} ctl 0 SW")
        else: L.append(f"R{k} n{k} n{k+1} {100*(1+0.1*rng.random()):.6g}")
        L.append(f"C{k} n{k+1} 0 {1e-9*(1+0.1*rng.random()):.6g}")
        if rng.random() < 0.5: L.append(f"D{k} n{k+1} 0 DM")
    L += [".tran 1e-6 7e-5", ".end", ""]
    ckt = parseNetlist("\n".join(L))
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    assert steps >= STEPS
    flat = abi.flatten(ckt).replicate(4)
    for j in range(4):  # four distinct instances of the one topology
        flat.R_val[j] *= 1.0 + 0.02 * j
        flat.C_val[j] *= 1.0 - 0.01 * j
    return flat, dt, abi.source_table(ckt, dt, steps)[: STEPS + 1]


CASES = {
    "diode_chain_1000": lambda: _chain("diode_chain", 1000),   # 512 row records in the streamed level: every lane has one
    "diode_chain_600": lambda: _chain("diode_chain", 600),     # fewer rows than threads
    "rc_ladder_1000": lambda: _chain("rc_ladder", 1000),       # factor reuse: right-hand-side-only records from step 1
    "switched_ladder": _switched_ladder,                       # a switch flips during the run: iterations > 1
}


def _run(flat, dt, src, geometry):
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=geometry)
    try:
        r = h.run(STEPS, dt, src)
        assert r["status"] == 0, r["detail"]
        return r, h.info()
    finally:
        h.close()


@pytest.mark.parametrize("no_table", [False, True], ids=["table", "no_table"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_packed_geometry_same_bits_as_latency_geometry(case, no_table, oracle_backend, monkeypatch):
    if no_table: monkeypatch.setenv("SPICEY_NO_PHASE_TABLE", "1")
    else: monkeypatch.delenv("SPICEY_NO_PHASE_TABLE", raising=False)
    flat, dt, src = CASES[case]()
    assert flat.n_inst == 4
    packed, info = _run(flat, dt, src, 2)
    latency, info1 = _run(flat, dt, src, 1)
    assert info["geometry"] == 2 and info["threads"] == 512 and info["resident_slots"] == 4 and info1["geometry"] == 1
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(packed[k], latency[k], equal_nan=(k != "iters")), (case, k)
    if case == "diode_chain_1000":
        assert info["streamed_tasks"] == 2000 and info["resident_tasks"] == 2719
    if case == "switched_ladder":
        assert flat.nS > 0 and int(packed["iters"].max()) > 1
    one = instance(flat, 2)
    ref = oracle_backend.run(one, STEPS, dt, src)
    assert ref["status"] == 0
    assert tol_ratio(packed["out_v"][2], ref["out_v"][0]).max() <= 1.0 and tol_ratio(packed["out_i"][2], ref["out_i"][0]).max() <= 1.0
    if flat.nS > 0:
        assert np.array_equal(packed["iters"][2], ref["iters"][0])
