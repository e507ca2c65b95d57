"""The launch plan's decision for the register-exchange top (tran_v2_run.h: TR) on the CPU, through spicey_plan itself
(tests/top_host): the circuits of tests/test_top_regs_gpu.py — every top size, the switched ladder, the batch, the chain
with a cut-off node — take the form by default and not with SPICEY_NO_TOP_REGS; a handle with two instances per
workgroup, the latency geometry, a plan without operand addresses and a run beyond the ready-argument kernel's step range
do not; and the decision function at the edges of the stage count (1 .. 6 stages = 2 .. 64 rows).  The form itself is GPU
code: host executors run spicey_pcr_stage whatever the build, so there is nothing of it to emulate here."""
from __future__ import annotations

import pytest

from spicey_amd import synth
from test_packed_resident_gpu import _switched_ladder
from top_host import pytop

STEPS = 64
KNOB = "SPICEY_NO_TOP_REGS"
KNOBS = (KNOB, "SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL")
# diode_chain length -> (rows of its top, stages): the lengths of tests/test_top_regs_gpu.py
TOP_ROWS = {22: (15, 4), 26: (16, 4), 31: (17, 5), 54: (32, 5), 63: (33, 6), 94: (63, 6), 110: (64, 6), 1000: (64, 6)}


def _chain(n, seeds=(1, 2)):
    flat, _, total, _ = synth.chain_batch("diode_chain", n, list(seeds), tran=f".tran 1e-6 {(STEPS + 6) * 1e-6:.6g}")
    assert total >= STEPS
    return flat


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _taken(p):
    return (p["rc"], p["top_regs"], p["top_regs_run"])


@pytest.mark.parametrize("n", sorted(TOP_ROWS))
def test_every_top_size_takes_the_form_and_the_knob_refuses_it(n, no_knobs):
    flat = _chain(n)
    on = pytop.plan(flat, steps=STEPS, geometry=2)
    assert _taken(on) == (0, 1, 1) and (on["pcr_rows"], on["stages"]) == TOP_ROWS[n]
    assert (on["packed"], on["fresh"], on["threads"], on["inst_per_wg"], on["addr"], on["addr_run"]) == (1, 1, 512, 1, 1, 1)
    no_knobs.setenv(KNOB, "1")
    off = pytop.plan(flat, steps=STEPS, geometry=2)
    assert _taken(off) == (0, 0, 0)
    # the same plan otherwise: the operand-address kernel, the same LDS (the two row buffers stay allocated)
    assert {k: v for k, v in off.items() if not k.startswith("top_regs")} == {k: v for k, v in on.items() if not k.startswith("top_regs")}


def test_the_smallest_top_has_fifteen_rows(no_knobs):
    """The symbolic phase builds no smaller top (so the 1-, 2- and 3-stage forms of the unrolled top run on no handle)."""
    rows = {pytop.plan(_chain(n, seeds=(1,)), steps=STEPS, geometry=2)["pcr_rows"] for n in range(2, 27)}
    assert rows == {0, 15, 16}


def test_the_switched_ladder_and_the_batch(no_knobs):
    flat, _, _ = _switched_ladder()
    p = pytop.plan(flat, steps=STEPS, geometry=2)
    assert _taken(p) == (0, 1, 1) and p["pcr_rows"] == 64 and flat.nS > 0
    p = pytop.plan(_chain(63, seeds=(3, 4, 5)), steps=STEPS, geometry=2)
    assert _taken(p) == (0, 1, 1) and p["pcr_rows"] == 33


def test_the_form_rides_on_the_operand_address_run(no_knobs):
    flat = _chain(63)
    # two instances per workgroup, and the latency geometry: another kernel
    k2 = pytop.plan(flat, steps=STEPS, inst_per_wg=2)
    assert _taken(k2) == (0, 0, 0) and k2["inst_per_wg"] == 2
    lat = pytop.plan(flat, steps=STEPS, geometry=1)
    assert _taken(lat) == (0, 0, 0) and lat["packed"] == 0 and lat["pcr_rows"] == 33
    # a run the ready-argument kernel does not take has no form above it either
    beyond = pytop.plan(flat, steps=2**32 - 1, geometry=2)
    assert (beyond["top_regs"], beyond["addr_run"], beyond["top_regs_run"]) == (1, 0, 0)
    # the knobs of the forms below it
    for knob in KNOBS[1:]:
        no_knobs.setenv(knob, "1")
        p = pytop.plan(flat, steps=STEPS, geometry=2)
        assert p["rc"] == 0 and p["top_regs_run"] == 0, knob
        if knob == "SPICEY_NO_OPERAND_ADDR":
            assert (p["addr"], p["top_regs"]) == (0, 0)
        no_knobs.delenv(knob)
    assert _taken(pytop.plan(flat, steps=STEPS, geometry=2)) == (0, 1, 1)


def test_the_decision_at_the_edges_of_the_stage_count(no_knobs):
    sh = pytop.shapes()
    want = {0: 0, 1: 0, 2: 1, 3: 2, 4: 2, 5: 3, 8: 3, 9: 4, 15: 4, 16: 4, 17: 5, 32: 5, 33: 6, 63: 6, 64: 6, 65: 7, 128: 7}
    for rows, stages in want.items():
        d = pytop.decide(True, rows)
        take = int(1 <= stages <= 6)
        assert (d["stages"], d["top_regs"], d["top_regs_run"], d["shape_top_regs"]) == (stages, take, take, 1), rows
        assert pytop.decide(False, rows)["top_regs"] == 0  # no operand addresses, no register exchange
    # the other shapes have no such kernel
    for name in ("packed_default", "latency"):
        assert sh[name] >= 0 and sh[name] != sh["packed_fresh"]
        d = pytop.decide(True, 64, shape=sh[name])
        assert (d["shape_top_regs"], d["top_regs"], d["top_regs_run"]) == (0, 0, 0), name
    assert pytop.decide(True, 64, shape=-1)["top_regs"] == 0
    no_knobs.setenv(KNOB, "1")
    assert pytop.decide(True, 64) == {"top_regs": 0, "stages": 6, "top_regs_run": 0, "shape_top_regs": 1}
