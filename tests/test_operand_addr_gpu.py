"""Operand-address kernel (tran_v2_run.h: OA — the always-executed LDS operands of the interpreter, of Z and of B are
addressed in one instruction from their record, terminal or descriptor word; B's descriptor fields index from the start
of the workspace) on the GPU against the same shape's ready-argument kernel: every case runs with SPICEY_NO_OPERAND_ADDR
set and without it and must give the same bits — voltages, currents, iteration counts, end state — and the run without
the knob is held against the oracle at the project's bar (1e-9 |ref| + 1e-12).  Every case also says which kernel it
expects: SpiceyInfo.interpreter and SpiceyInfo.operand_addr of the handle, and the launch's own decision for the run
(spicey_addr_run, through the plan harness).  Small shapes on purpose: a wrong half, a wrong base or a stale re-encoding
changes bits at any size."""
from __future__ import annotations

import numpy as np
import pytest

from addr_host import pyaddr
from batch_variants import instance
from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist
from test_early_prefetch_gpu import _against_oracle, _same_bits, _switched
from test_ready_args_gpu import _inductor_chain

pytestmark = pytest.mark.gpu

KNOB = "SPICEY_NO_OPERAND_ADDR"
OTHER_KNOBS = ("SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL", "SPICEY_FRESH_FILL_LINEAR")


def _chain(kind, n, seeds, steps):
    flat, dt, total, src = synth.chain_batch(kind, n, list(seeds), tran=f".tran 1e-6 {(steps + 6) * 1e-6:.6g}")
    assert total >= steps
    return flat, dt, src[: steps + 1], steps


def _grounded_both_ways(n=150, steps=40):
    """A diode chain in which ground stands on BOTH terminal positions of resident items of every class: every third
    resistor, capacitor and diode is written with ground first (the diodes then point up from ground, clamping negative
    swings of the bipolar source), and shunt resistors to ground alternate their direction too."""
    L = ["* ground on both terminal positions", ".model DM D(Is=1e-14 N=1)", "V1 n1 0 PULSE(-3 5 0 1e-6 1e-6 4e-6 1e-5)"]
    for k in range(1, n):
        L.append(f"R{k} n{k} n{k+1} {100 * (1 + 0.001 * (k % 17)):.6g}")
        if k % 3 == 0: L.append(f"C{k} 0 n{k+1} {1e-9 * (1 + 0.002 * (k % 11)):.6g}")
        else: L.append(f"C{k} n{k+1} 0 {1e-9 * (1 + 0.002 * (k % 11)):.6g}")
        if k % 3 == 1: L.append(f"D{k} 0 n{k+1} DM")
        else: L.append(f"D{k} n{k+1} 0 DM")
        if k % 4 == 0: L.append(f"RS{k} 0 n{k+1} {1e4 * (1 + 0.01 * (k % 5)):.6g}")
        if k % 4 == 2: L.append(f"RT{k} n{k+1} 0 {2e4 * (1 + 0.01 * (k % 7)):.6g}")
    L += [f".tran 1e-6 {(steps + 6) * 1e-6:.6g}", ".end", ""]
    ckt = parseNetlist("\n".join(L))
    dt, total = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt).replicate(2)
    flat.R_val[1] *= 1.03
    assert total >= steps
    # ground (node 0) on the first and on the second terminal position of every element class
    for a, b in ((flat.R_n1, flat.R_n2), (flat.C_n1, flat.C_n2), (flat.D_np, flat.D_nm)):
        assert (np.asarray(a) == 0).any() and (np.asarray(b) == 0).any()
    return flat, dt, abi.source_table(ckt, dt, total)[: steps + 1], steps


def _switched_case():
    flat, dt, src, steps = _switched()
    return flat, dt, src, steps


# name: (circuit, the handle takes the operand-address kernel)
CASES = {
    "diode_chain_100_x4_200": (lambda: _chain("diode_chain", 100, (1, 2, 3, 4), 200), True),   # most threads own no item; instances 0..3
    "diode_chain_1000_x2_64": (lambda: _chain("diode_chain", 1000, (1, 2), 64), True),         # every resident item exists, every lane has a row record
    "rc_ladder_100": (lambda: _chain("rc_ladder", 100, (1, 2), 40), False),                    # linear: the default program, another shape
    "inductor_chain": (_inductor_chain, True),                                                 # Z's inductor loop beside the handles
    "switched_ladder": (_switched_case, True),                                                 # a_reiterate between OA phases
    "grounded_both_ways": (_grounded_both_ways, True),                                         # the +0.0 slot in either half
}


def _run(flat, dt, src, steps, runs=(None,), **kw):
    """-> the results of `runs` (step counts, None: `steps`) on ONE handle, and its info()"""
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=2)
    try:
        out = []
        for n in runs:
            n = steps if n is None else n
            r = h.run(n, dt, src[: n + 1], **kw)
            assert r["status"] == 0, r["detail"]
            out.append(r)
        return out, h.info()
    finally:
        h.close()


def _both(monkeypatch, flat, dt, src, steps, want, **kw):
    """Knob on (the ready-argument kernel), knob off (the operand-address kernel where the plan says so); what each handle
    reports and what each run launched."""
    for k in OTHER_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(KNOB, "1")
    off, info_off = _run(flat, dt, src, steps, **kw)
    p_off = pyaddr.plan(flat, steps=steps, geometry=2)
    monkeypatch.delenv(KNOB)
    on, info_on = _run(flat, dt, src, steps, **kw)
    p_on = pyaddr.plan(flat, steps=steps, geometry=2)
    assert info_on["interpreter"] == 2 and info_off["interpreter"] == 2
    assert info_off["operand_addr"] == 0 and p_off["rc"] == 0 and p_off["addr_run"] == 0
    assert info_on["operand_addr"] == int(want) and p_on["rc"] == 0 and p_on["addr_run"] == int(want) and p_on["info_operand_addr"] == int(want)
    assert {k: v for k, v in info_on.items() if k != "operand_addr"} == {k: v for k, v in info_off.items() if k != "operand_addr"}  # the same plan, the same LDS
    if want:
        assert info_on["geometry"] == 2 and info_on["threads"] == 512 and info_on["resident_slots"] == 4 and p_on["ready_run"] == 1
    return off, on, info_on


@pytest.mark.parametrize("case", sorted(CASES))
def test_knob_off_and_on_give_the_same_bits_and_the_oracles_values(case, oracle_backend, monkeypatch):
    make, want = CASES[case]
    flat, dt, src, steps = make()
    off, on, info = _both(monkeypatch, flat, dt, src, steps, want)
    _same_bits(off[0], on[0], case)
    if case == "switched_ladder":
        assert flat.nS > 0 and int(on[0]["iters"].max()) > 1
    if case == "rc_ladder_100":
        assert info["factor_reuse"] == 1  # (why the plan kept the default program)
    if case == "inductor_chain":
        assert flat.nL > 0
    for j in sorted({0, flat.n_inst - 1}):
        _against_oracle(oracle_backend, on[0], instance(flat, j), j, steps, dt, src, flat.nS > 0)


def test_a_run_without_currents(oracle_backend, monkeypatch):
    flat, dt, src, steps = _chain("diode_chain", 100, (1, 2), 40)
    off, on, _ = _both(monkeypatch, flat, dt, src, steps, True, want_currents=False)
    got, ref0 = on[0], off[0]
    assert got["out_i"] is None and ref0["out_i"] is None
    assert np.array_equal(got["out_v"], ref0["out_v"]) and np.array_equal(got["iters"], ref0["iters"])
    for k, v in ref0["state"].items():
        assert np.array_equal(np.asarray(v), np.asarray(got["state"][k])), k
    ref = oracle_backend.run(instance(flat, 1), steps, dt, src)
    from test_gpu_parity import tol_ratio
    assert ref["status"] == 0 and tol_ratio(got["out_v"][1], ref["out_v"][0]).max() <= 1.0


def test_two_runs_on_one_handle(oracle_backend, monkeypatch):
    """The second run starts from the first one's end state; its prologue re-encodes the descriptors again, from the
    program's own (a field re-encoded twice would name an operand nW further on)."""
    flat, dt, src, steps = _chain("diode_chain", 100, (1, 2), 40)
    first, second = steps, 17
    off, on, _ = _both(monkeypatch, flat, dt, src, steps, True, runs=(first, second))
    for r in (0, 1):
        _same_bits(off[r], on[r], f"run {r}")
    assert on[1]["out_v"].shape[1] == second + 1 and not np.array_equal(on[0]["out_v"][:, : second + 1], on[1]["out_v"])  # (the state did carry over)
    j = 1
    ref0 = _against_oracle(oracle_backend, on[0], instance(flat, j), j, first, dt, src[: first + 1], False)
    nxt = instance(flat, j)
    for k in ("C_vprev", "L_iprev", "D_vdprev"):
        setattr(nxt, k, np.array(ref0["state"][k], dtype=np.float64).reshape(getattr(nxt, k).shape))
    _against_oracle(oracle_backend, on[1], nxt, j, second, dt, src[: second + 1], False)
