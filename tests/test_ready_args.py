"""Ready-argument builds (tran_v2_run.h: RA) on the CPU: the packed layout (512 threads, 4 slots) of the fresh operand-slot
build whose Z and early fetch move only their hot arguments to scalars, read the rest inside the branch that needs it,
take the record, the source table and the iteration counts from pointers that the prologue made the instance's own, and
form step x row as a 32 x 32 -> 64-bit product — against the same build without all that: same bits in voltages,
currents, iteration counts and end state, also with the threads of every phase in reverse order and from an arena that
starts as NaN.  The rebased words of the table are held against their formulas for instance 0 and a later instance.
Also the launch plan's decision, with and without SPICEY_NO_READY_ARGS and for a run whose step count is outside the
condition of the product.

The harness is tests/ready_host (it compiles the emulator's sources unchanged and runs every workgroup in one arena laid
out like the kernel's LDS)."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import synth

from batch_variants import instance
from ready_host import pyready
from test_packed_resident_gpu import _switched_ladder

STEPS = 64


def _chain(n, seeds=(3,)):
    flat, dt, steps, src = synth.chain_batch("diode_chain", n, list(seeds), tran=".tran 1e-6 7e-5")
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


def _switched_one():
    flat, dt, src = _switched_ladder()
    return instance(flat, 2), dt, src


CASES = {
    "diode_chain_100": lambda: _chain(100),     # most threads own no item
    "diode_chain_1000": lambda: _chain(1000),   # the bench circuit
    "switched_ladder": _switched_one,           # B and the solve run twice in a step; Z's switch loop takes the complete structs
}
_OFF: dict = {}


def _off_run(case):
    """The operand-slot build without ready arguments: computed once per case, never modified."""
    if case not in _OFF:
        flat, dt, src = CASES[case]()
        r = pyready.run(flat, STEPS, dt, src, ready=False)
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
def test_ready_arguments_give_the_bits_of_the_full_head(case, nan_fill):
    flat, dt, src, ref = _off_run(case)
    got = pyready.run(flat, STEPS, dt, src, ready=True, nan_fill=nan_fill)
    assert got["status"] == 0 and got["slots_fit"] == 1 and got["pcr_n"] > 0
    assert np.isfinite(got["out_v"]).all() and np.isfinite(got["out_i"]).all()
    _same(got, ref, case)
    assert int(got["iters"].min()) >= 1  # (every step's count was written through the instance's own row)
    if case == "switched_ladder":
        assert got["nS"] > 0 and int(got["iters"].max()) > 1
    # the end state went through the lazily read pointers of the last step
    assert not np.array_equal(got["state"]["C_vprev"], flat.C_vprev)


@pytest.mark.parametrize("case", ["diode_chain_100", "switched_ladder"])
def test_thread_order_within_a_phase_does_not_matter(case):
    flat, dt, src, ref = _off_run(case)
    got = pyready.run(flat, STEPS, dt, src, ready=True, reverse=True, nan_fill=True)
    assert got["status"] == 0
    _same(got, ref, "reversed")


def _u64(row, i):
    return int(row[i]) | (int(row[i + 1]) << 32)


def test_rebased_words_follow_their_formulas():
    """Three instances, each with a source table of its own (src_stride != 0)."""
    flat, dt, src = _chain(100, seeds=(3, 4, 5))
    ni = flat.n_inst
    assert ni == 3
    per = np.stack([src * (1.0 + 0.1 * g) for g in range(ni)])
    on = pyready.run(flat, STEPS, dt, per, ready=True)
    off = pyready.run(flat, STEPS, dt, per, ready=False)
    assert on["status"] == 0 and off["status"] == 0 and on["src_stride"] == (STEPS + 1) * on["nV"] > 0
    _same(on, off, "per-instance sources")
    assert not np.array_equal(on["out_v"][0], on["out_v"][2])
    w = pyready.words()
    for g in (0, 2):
        t, a = on["table"][g], on["addr"]
        assert _u64(t, w["ZPAR"]) == a["zpar"] + g * on["zrec"] * 8
        assert _u64(t, w["SRC"]) == a["src"] + g * on["src_stride"] * 8
        assert _u64(t, w["ITERS"]) == a["iters"] + g * (STEPS + 1) * 4
        assert _u64(t, w["OUT_V"]) == a["out_v"] + g * (STEPS + 1) * on["nOut"] * 8
        assert _u64(t, w["OUT_I"]) == a["out_i"] + g * (STEPS + 1) * on["nCur"] * 8
        # what Z reads inside its last-step branch is the array itself: Z indexes it by instance
        assert _u64(t, w["C_VPREV"]) == a["C_vprev"] and _u64(t, w["D_VDPREV"]) == a["D_vdprev"]
        # the build without ready arguments leaves the three pointers as the run gave them
        to, ao = off["table"][g], off["addr"]
        assert _u64(to, w["ZPAR"]) == ao["zpar"] and _u64(to, w["SRC"]) == ao["src"] and _u64(to, w["ITERS"]) == ao["iters"]
    # the counts of the block (words 0-7 and 14-17) are the same in both builds
    same = list(range(8)) + [14, 15, 16, 17]
    assert np.array_equal(on["table"][2][same], off["table"][2][same])


def test_a_null_current_pointer_stays_null():
    flat, dt, src, ref = _off_run("diode_chain_100")
    got = pyready.run(flat, STEPS, dt, src, ready=True, currents=False)
    assert got["status"] == 0 and _u64(got["table"][0], pyready.words()["OUT_I"]) == 0
    assert np.array_equal(got["out_v"], ref["out_v"]) and np.array_equal(got["iters"], ref["iters"])
    for k, v in ref["state"].items():
        assert np.array_equal(got["state"][k], v), k


def test_plan_takes_ready_arguments_and_the_knob_and_the_step_count_keep_the_other_kernel(monkeypatch):
    flat, _, _ = _chain(1000)
    flat = flat.replicate(3)
    for k in ("SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL"):
        monkeypatch.delenv(k, raising=False)
    on = pyready.plan(flat, steps=10000, geometry=2)
    assert on["rc"] == 0 and (on["packed"], on["fresh"], on["early"], on["slots"], on["ready"], on["ready_run"], on["threads"]) == (1, 1, 1, 1, 1, 1, 512)
    # the condition of the 32 x 32 -> 64-bit product: step + 1 fits 32 bits for every step of the run
    assert pyready.plan(flat, steps=2**32 - 2, geometry=2)["ready_run"] == 1
    for steps in (2**32 - 1, 2**32, 2**40):
        p = pyready.plan(flat, steps=steps, geometry=2)
        assert (p["ready"], p["slots"], p["ready_run"]) == (1, 1, 0)  # the same handle, the operand-slot kernel for this run
    monkeypatch.setenv("SPICEY_NO_READY_ARGS", "1")
    off = pyready.plan(flat, steps=10000, geometry=2)
    assert off["rc"] == 0 and (off["packed"], off["fresh"], off["early"], off["slots"], off["ready"], off["ready_run"]) == (1, 1, 1, 1, 0, 0)
    assert off["lds_bytes"] == on["lds_bytes"]
    monkeypatch.delenv("SPICEY_NO_READY_ARGS")
    # the form rides on the operand-slot kernel: without it, none
    monkeypatch.setenv("SPICEY_NO_OPERAND_SLOTS", "1")
    p = pyready.plan(flat, steps=10000, geometry=2)
    assert (p["slots"], p["ready"], p["ready_run"]) == (0, 0, 0)
    monkeypatch.delenv("SPICEY_NO_OPERAND_SLOTS")
    lat = pyready.plan(flat, steps=10000, geometry=1)
    assert lat["rc"] == 0 and (lat["packed"], lat["ready"], lat["ready_run"]) == (0, 0, 0)
