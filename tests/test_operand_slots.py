"""Operand-slot builds (tran_v2_phases.h: OS) on the CPU: the packed layout (512 threads, 4 slots) of the fresh early-prefetch
build with ground resolved to the +0.0 slot in Z's resident terminal indices, Z's stores on per-section bases, the row
bases taken from the phase table, and B's resident descriptors naming the -0.0 slot in every empty field, against the same
build without the slots — same bits in voltages, currents, iteration counts and end state, also with the threads of every
phase in reverse order and from an arena that starts as NaN.  Both slots must hold their constants after a run (compared
by bit pattern: -0.0 == 0.0).  Also the slot positions and the launch plan's decision, with and without
SPICEY_NO_OPERAND_SLOTS and for programs without room.

The harness is tests/slots_host (it compiles the emulator's sources unchanged and runs every workgroup in one arena laid
out like the kernel's LDS).  A conductance stamp enters a diagonal with + and an off-diagonal entry with -, so no entry
of a netlist carries two conductances of OPPOSITE sign; dense_rows has entries of two conductances and rows of four
contributions with both signs."""
from __future__ import annotations

import struct

import numpy as np
import pytest

from spicey_amd import synth

from batch_variants import instance
from slots_host import circuits, pyslots
from test_packed_resident_gpu import _switched_ladder

STEPS = 64
PLUS_ZERO = struct.unpack("<q", struct.pack("<d", 0.0))[0]
MINUS_ZERO = struct.unpack("<q", struct.pack("<d", -0.0))[0]


def _chain(n):
    flat, dt, steps, src = synth.chain_batch("diode_chain", n, [3], tran=".tran 1e-6 7e-5")
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


def _switched_one():
    flat, dt, src = _switched_ladder()
    return instance(flat, 2), dt, src


def _reversed(n, both_grounds=False):
    flat, dt, steps, src = circuits.reversed_chain(n, both_grounds=both_grounds)
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


def _dense(n):
    flat, dt, steps, src = circuits.dense_rows(n)
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


CASES = {
    "diode_chain_100": lambda: _chain(100),      # most threads own no item: their indices all name the +0.0 slot
    "diode_chain_333": lambda: _chain(333),      # counts that are no multiple of a wave
    "diode_chain_1023": lambda: _chain(1023),    # the largest chain of the shape: every resident item exists
    "switched_ladder": _switched_one,            # B and the solve run twice in a step
    "reversed_chain_200": lambda: _reversed(200),              # ground is terminal a: (+0.0) - v
    "two_grounds": lambda: _reversed(60, both_grounds=True),   # an element between ground and ground: (+0.0) - (+0.0)
    "dense_rows_200": lambda: _dense(200),       # rows of four contributions with both signs, entries of two conductances, and the list forms of both
}
_OFF: dict = {}


def _off_run(case):
    """The build without the slots: computed once per case, never modified."""
    if case not in _OFF:
        flat, dt, src = CASES[case]()
        r = pyslots.run(flat, STEPS, dt, src, slots=False)
        assert r["status"] == 0 and r["fresh_fill"] == 1
        for a in (r["out_v"], r["out_i"], r["iters"], *r["state"].values()):
            a.setflags(write=False)
        _OFF[case] = (flat, dt, src, r)
    return _OFF[case]


def _same(got, ref, what):
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    for k, v in ref["state"].items():
        assert np.array_equal(got["state"][k], v), (what, k)


@pytest.mark.parametrize("nan_fill", [False, True], ids=["zeroed", "nan_arena"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_slots_give_the_bits_of_compare_and_select(case, nan_fill):
    flat, dt, src, ref = _off_run(case)
    got = pyslots.run(flat, STEPS, dt, src, slots=True, nan_fill=nan_fill)
    assert got["status"] == 0 and got["slots_fit"] == 1 and got["pcr_n"] > 0
    assert np.isfinite(got["out_v"]).all() and np.isfinite(got["out_i"]).all()
    _same(got, ref, case)
    # the two constants, by bit pattern, after the last step
    assert got["bits_plus"] == PLUS_ZERO and got["bits_minus"] == MINUS_ZERO
    if case == "switched_ladder":
        assert got["nS"] > 0 and int(got["iters"].max()) > 1
    if case == "diode_chain_1023":
        assert flat.nR == flat.nC == flat.nD == 1022 and flat.n_out == 1023  # (two items of every kind on all but one or two of 512 threads)
    if case in ("reversed_chain_200", "two_grounds"):
        assert (np.asarray(flat.D_np) == 0).all() and float(np.abs(ref["out_i"][0, :, -flat.nD:]).max()) > 1e-6  # ground first, and the diodes conduct
    if case == "two_grounds":
        assert ((np.asarray(flat.R_n1) == 0) & (np.asarray(flat.R_n2) == 0)).any()


def test_thread_order_within_a_phase_does_not_matter():
    flat, dt, src, ref = _off_run("reversed_chain_200")
    got = pyslots.run(flat, STEPS, dt, src, slots=True, reverse=True, nan_fill=True)
    assert got["status"] == 0
    _same(got, ref, "reversed")
    assert got["bits_plus"] == PLUS_ZERO and got["bits_minus"] == MINUS_ZERO


def test_slot_positions():
    # the bench circuit's order of magnitude: the slots are the last two doubles of the workgroup's LDS
    w = pyslots.where(nW=7000, nU=3001, nGdyn=999, nS=0, pcr_n=40, pcr_level=3)
    assert w["fit"] == 1 and w["end_bytes"] == w["lds_bytes"]
    # ... whatever the alignment of the sections in front of them
    for nS in (0, 1, 2, 3, 5):
        w = pyslots.where(nW=701, nU=33, nGdyn=7, nS=nS, pcr_n=17, pcr_level=2)
        assert w["fit"] == 1 and w["end_bytes"] == w["lds_bytes"] and w["slot_index"] * 8 + 16 == w["lds_bytes"]
    # the table's rows reach the last four words of the tail area: the table fits (64 rows of the top, 5 levels), the slots do not
    assert pyslots.where(7000, 3001, 999, 0, pcr_n=64, pcr_level=4)["fit"] == 1
    assert pyslots.where(7000, 3001, 999, 0, pcr_n=64, pcr_level=5)["fit"] == 0
    # no table: no top, a top of more than a wave, tail records in the area
    assert pyslots.where(7000, 3001, 999, 0, pcr_n=0, pcr_level=0)["fit"] == 0
    assert pyslots.where(7000, 3001, 999, 0, pcr_n=65, pcr_level=2)["fit"] == 0
    assert pyslots.where(7000, 3001, 999, 0, pcr_n=40, pcr_level=3, tail_n=6)["fit"] == 0
    # beyond the reach of phase B's 14-bit descriptor fields, which count from the start of the element vectors
    assert pyslots.where(nW=7000, nU=12000, nGdyn=3600, nS=0, pcr_n=40, pcr_level=3)["fit"] == 1
    assert pyslots.where(nW=7000, nU=12000, nGdyn=3700, nS=0, pcr_n=40, pcr_level=3)["fit"] == 0
    # beyond the reach of a 16-bit index (0xFFFF itself still means ground where a pair comes from global memory)
    near = pyslots.where(nW=60000, nU=4000, nGdyn=1000, nS=0, pcr_n=40, pcr_level=3)
    assert near["slot_index"] + 1 >= 0xFFFF and near["fit"] == 0


def test_plan_takes_the_slots_where_they_fit_and_the_knobs_keep_the_other_kernels(monkeypatch):
    flat, _, _ = _chain(1000)
    flat = flat.replicate(3)
    for k in ("SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL"):
        monkeypatch.delenv(k, raising=False)
    on = pyslots.plan(flat, geometry=2)
    assert on["rc"] == 0 and (on["packed"], on["fresh"], on["early"], on["slots"], on["threads"]) == (1, 1, 1, 1, 512)
    monkeypatch.setenv("SPICEY_NO_OPERAND_SLOTS", "1")
    off = pyslots.plan(flat, geometry=2)
    assert off["rc"] == 0 and (off["packed"], off["fresh"], off["early"], off["slots"]) == (1, 1, 1, 0)
    assert off["lds_bytes"] == on["lds_bytes"]  # the slots take space that was reserved already
    monkeypatch.delenv("SPICEY_NO_OPERAND_SLOTS")
    # the slots lie behind the phase table and ride on the early-prefetch kernel: without either, none
    monkeypatch.setenv("SPICEY_NO_PHASE_TABLE", "1")
    assert pyslots.plan(flat, geometry=2)["slots"] == 0
    monkeypatch.delenv("SPICEY_NO_PHASE_TABLE")
    monkeypatch.setenv("SPICEY_NO_EARLY_PREFETCH", "1")
    assert pyslots.plan(flat, geometry=2)["slots"] == 0
    monkeypatch.delenv("SPICEY_NO_EARLY_PREFETCH")
    # a shape without such a kernel: the 6-entry packed build, the latency geometry
    monkeypatch.setenv("SPICEY_NO_FRESH_FILL", "1")
    assert pyslots.plan(flat, geometry=2)["slots"] == 0
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL")
    lat = pyslots.plan(flat, geometry=1)
    assert lat["rc"] == 0 and (lat["packed"], lat["slots"]) == (0, 0)
