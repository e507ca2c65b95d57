"""Register-exchange top (tran_v2_run.h: TR — the tridiagonal top of the packed operand-address kernel keeps its rows in
registers and reads its neighbours' rows from their lanes instead of through the two LDS row buffers) on the GPU against
the same library with SPICEY_NO_TOP_REGS: every case runs both ways on the packed layout (512 threads, 4 slots), 64 steps,
all voltages and currents, and must give the same bits — voltages, currents, iteration counts, status, solve count, end
state; the run without the knob is held against the emulator of this very build (tests/addr_host: the fresh
operand-address build on the sequential executor, whose top is spicey_pcr_stage) at the project's bar, 1e-9 |ref| + 1e-12.
Every case says which form it expects (spicey_top_regs_form of the handle, and the plan's own decision on the CPU).

Top sizes.  The symbolic phase builds no top below 15 rows (symbolic.cpp: `cnt >= 15`), so tops of 2 and 3 rows do not
exist on any handle; the smallest is 15.  The chain lengths below were found on the CPU (tests/top_host, pcr_rows of the
plan, diode_chain(n) for n = 2 .. 1100) and are the shapes where end clamping (a neighbour index clamped at lane 0 / 63),
identity rows (lanes past the last row) and the number of stages differ:
  n = 22 -> 15 rows (S = 4, the smallest top), 26 -> 16 (2^4), 31 -> 17 (S = 5, one past), 54 -> 32 (2^5),
  63 -> 33 (S = 6, one past), 94 -> 63, 110 -> 64 (every lane a row: no identity row; all longer chains have 64 too)."""
from __future__ import annotations

import numpy as np
import pytest

from addr_host import pyaddr
from batch_variants import instance
from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist
from test_gpu_parity import tol_ratio
from test_packed_resident_gpu import _switched_ladder
from top_host import pytop

pytestmark = pytest.mark.gpu

STEPS = 64
KNOB = "SPICEY_NO_TOP_REGS"
OTHER_KNOBS = ("SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL",
               "SPICEY_FRESH_FILL_LINEAR")
# diode_chain length -> rows of its top (see the module's docstring)
TOP_ROWS = {22: 15, 26: 16, 31: 17, 54: 32, 63: 33, 94: 63, 110: 64}


def _chain(n, seeds=(1, 2)):
    flat, dt, total, src = synth.chain_batch("diode_chain", n, list(seeds), tran=f".tran 1e-6 {(STEPS + 6) * 1e-6:.6g}")
    assert total >= STEPS
    return flat, dt, src[: STEPS + 1]


def _run(flat, dt, src, **options):
    """-> (result of one run of STEPS steps, info(), spicey_top_regs_form for that run) of a fresh handle"""
    from spicey_amd.lib import Handle
    h = Handle(flat, **options)
    try:
        form = h.top_regs_form(STEPS)
        r = h.run(STEPS, dt, src)
        return r, h.info(), form
    finally:
        h.close()


def _both(monkeypatch, flat, dt, src, want=True, **options):
    """Knob set (the rows go through LDS), knob not set (the register exchange where the plan says so): what each handle
    reports, and the same plan otherwise."""
    options.setdefault("geometry", 2)
    for k in OTHER_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(KNOB, "1")
    off, info_off, form_off = _run(flat, dt, src, **options)
    p_off = pytop.plan(flat, steps=STEPS, **options)
    monkeypatch.delenv(KNOB)
    on, info_on, form_on = _run(flat, dt, src, **options)
    p_on = pytop.plan(flat, steps=STEPS, **options)
    assert info_on == info_off  # the same plan, the same LDS: the knob picks between two kernels of one shape
    assert form_off is False and p_off["rc"] == 0 and (p_off["top_regs"], p_off["top_regs_run"]) == (0, 0)
    assert form_on is bool(want) and p_on["rc"] == 0 and (p_on["top_regs"], p_on["top_regs_run"]) == (int(want), int(want))
    if want:
        assert (info_on["interpreter"], info_on["geometry"], info_on["threads"], info_on["resident_slots"], info_on["operand_addr"]) == (2, 2, 512, 4, 1)
        assert 2 <= info_on["pcr_rows"] <= 64 and p_on["addr_run"] == 1
    return off, on, info_on


def _same(off, on, what):
    assert on["status"] == off["status"] and on["detail"] == off["detail"], what
    assert np.array_equal(on["inst_status"], off["inst_status"]), what
    for k in ("out_v", "out_i"):
        assert np.array_equal(on[k], off[k], equal_nan=True), (what, k)
    assert np.array_equal(on["iters"], off["iters"]), (what, "iters")
    if on["status"] == 0:
        assert on["solves"] == off["solves"], what
        for k, v in off["state"].items():
            assert np.array_equal(np.asarray(v), np.asarray(on["state"][k]), equal_nan=(k != "S_ison")), (what, "state", k)


def _meets_emulator(got, flat, dt, src, what):
    ref = pyaddr.run(flat, STEPS, dt, src, addr=True)
    assert ref["status"] == 0 and ref["pcr_n"] > 0
    rv = float(tol_ratio(got["out_v"], ref["out_v"]).max())
    ri = float(tol_ratio(got["out_i"], ref["out_i"]).max())
    print(f"top-regs ratio {what}: out_v {rv:.3g} out_i {ri:.3g} of the bar")
    assert rv <= 1.0 and ri <= 1.0, (what, rv, ri)
    assert np.array_equal(got["iters"], ref["iters"]), what


@pytest.mark.parametrize("n", sorted(TOP_ROWS))
def test_every_top_size_gives_the_bits_of_the_lds_exchange(n, monkeypatch):
    flat, dt, src = _chain(n)
    off, on, info = _both(monkeypatch, flat, dt, src)
    assert info["pcr_rows"] == TOP_ROWS[n]
    assert on["status"] == 0, on["detail"]
    assert np.isfinite(on["out_v"]).all() and np.isfinite(on["out_i"]).all()
    _same(off, on, n)
    _meets_emulator(on, flat, dt, src, f"diode_chain({n})")


def test_the_bench_circuit(monkeypatch):
    flat, dt, src = _chain(1000)
    off, on, info = _both(monkeypatch, flat, dt, src)
    assert info["pcr_rows"] == 64 and on["status"] == 0
    _same(off, on, 1000)
    _meets_emulator(on, flat, dt, src, "diode_chain(1000)")


def test_a_switched_ladder_reiterates_through_the_top(monkeypatch):
    """B, the factor phases and the top run several times in a step, with a_reiterate between them; 4 instances."""
    flat, dt, src = _switched_ladder()
    src = src[: STEPS + 1]
    off, on, info = _both(monkeypatch, flat, dt, src)
    assert info["pcr_rows"] == 64 and on["status"] == 0
    assert flat.nS > 0 and int(on["iters"].max()) > 1
    _same(off, on, "switched ladder")
    _meets_emulator(on, flat, dt, src, "switched ladder")


def test_three_instances_with_their_own_sources(monkeypatch):
    flat, dt, src = _chain(63, seeds=(3, 4, 5))
    per = np.ascontiguousarray(np.stack([src * s for s in (1.0, 0.6, -0.4)]))  # (a bipolar one among them: the diodes stay off)
    assert per.shape == (3, STEPS + 1, flat.nV)
    off, on, info = _both(monkeypatch, flat, dt, per)
    assert info["pcr_rows"] == 33 and info["n_workgroups"] == 3 and on["status"] == 0
    _same(off, on, "three instances")
    assert not np.array_equal(on["out_v"][0], on["out_v"][1]) and not np.array_equal(on["out_v"][1], on["out_v"][2])
    _meets_emulator(on, flat, dt, per, "three instances, per-instance sources")


def _half_clamped_chain(n=110):
    """A chain with a diode at every other node only, three instances: a node without one can be cut off."""
    L = ["* chain, a diode at every other node", ".model DM D(Is=1e-14 N=1)", "V1 n1 0 PULSE(0 5 0 1e-6 1e-6 4e-6 1e-5)"]
    for k in range(1, n):
        L.append(f"R{k} n{k} n{k+1} {100 * (1 + 0.001 * (k % 17)):.6g}")
        L.append(f"C{k} n{k+1} 0 {1e-9 * (1 + 0.002 * (k % 11)):.6g}")
        if k % 2: L.append(f"D{k} n{k+1} 0 DM")
    L += [f".tran 1e-6 {(STEPS + 6) * 1e-6:.6g}", ".end", ""]
    ckt = parseNetlist("\n".join(L))
    dt, total = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    assert total >= STEPS
    return abi.flatten(ckt).replicate(3), dt, abi.source_table(ckt, dt, total)[: STEPS + 1]


def test_a_singular_pivot_in_the_top_is_reported_the_same_way(monkeypatch):
    """Instance 1 of three has node 55 cut off (its resistors 1e16 ohm, its capacitor 1e-30 F, no diode there): the row's
    pivot is ~2e-16, below the 1e-15 of the reference.  Node 55 is the middle separator of the 110-node chain (elimination
    level >= 5 of 8; the 64-row top holds every pivot above level 0), so it is the top's running minimum that trips
    flags[1] — an error return, not a fault.  Both forms must name the same instance, step and iteration, and the
    instances beside it must finish with the same bits."""
    flat, dt, src = _half_clamped_chain()
    node = 55
    assert node not in set(flat.D_np) | set(flat.D_nm) | set(flat.V_n1) | set(flat.V_n2)
    flat.R_val[1, (flat.R_n1 == node) | (flat.R_n2 == node)] = 1e16
    flat.C_val[1, (flat.C_n1 == node) | (flat.C_n2 == node)] = 1e-30
    per = np.ascontiguousarray(np.broadcast_to(src, (3, STEPS + 1, flat.nV)))  # (per-instance layout: partial results stand)
    off, on, info = _both(monkeypatch, flat, dt, per)
    assert info["pcr_rows"] == 64 and info["pcr_level"] == 1
    assert on["status"] == abi.ERR_SINGULAR and "singular at inst 1 step 0" in on["detail"]
    assert np.array_equal(on["inst_status"], [0, abi.ERR_SINGULAR, 0])
    assert on["detail"] == off["detail"] and np.array_equal(on["inst_status"], off["inst_status"])
    for j in (0, 2):
        for k in ("out_v", "out_i", "iters"):
            assert np.array_equal(on[k][j], off[k][j]), (j, k)
        assert np.isfinite(on["out_v"][j]).all()


def test_the_form_is_not_taken_where_its_conditions_fail(monkeypatch):
    for k in OTHER_KNOBS + (KNOB,):
        monkeypatch.delenv(k, raising=False)
    flat, dt, src = _chain(63)
    # by default on this shape
    on, _, form = _run(flat, dt, src, geometry=2)
    assert form is True and on["status"] == 0
    # the latency geometry has no such kernel
    lat, info, form = _run(flat, dt, src, geometry=1)
    assert form is False and info["geometry"] == 1 and lat["status"] == 0
    # two instances per workgroup: no operand addresses, no register exchange
    k2, info, form = _run(flat, dt, src, inst_per_wg=2)
    assert form is False and info["inst_per_wg"] == 2 and k2["status"] == 0
    # where the operand-address condition fails, the form below it runs and this one does not
    monkeypatch.setenv("SPICEY_NO_OPERAND_ADDR", "1")
    oa, info, form = _run(flat, dt, src, geometry=2)
    assert form is False and info["operand_addr"] == 0 and oa["status"] == 0
    monkeypatch.delenv("SPICEY_NO_OPERAND_ADDR")
    # a run beyond the ready-argument kernel's step range has neither form (asked of the handle, not run)
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=2)
    try:
        assert h.top_regs_form(STEPS) is True and h.top_regs_form(2**32 - 1) is False
    finally:
        h.close()
    # ... and all of them computed the same circuit: the packed ones bit for bit
    for r in (oa,):
        assert np.array_equal(r["out_v"], on["out_v"]) and np.array_equal(r["out_i"], on["out_i"]) and np.array_equal(r["iters"], on["iters"])
    for r in (lat, k2):
        assert tol_ratio(r["out_v"], on["out_v"]).max() <= 1.0
