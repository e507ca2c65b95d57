"""Early-prefetch builds (tran_v2_run.h: EP) on the CPU: the packed layout (512 threads, 4 slots) of the fresh build with Z's
parameters taken from the per-thread record SpiceyRun::zpar and fetched between the factor and the backward phases, against
the same build without the record — same bits, on both placements of the fetch (the peeled last factor phase of a plain
executor, the phase of the tridiagonal top of an executor with idle waves), also from a record, a workspace and prefetch
registers that start as NaN — and the launch plan's decision with and without SPICEY_NO_EARLY_PREFETCH.

The harness is tests/early_host (it compiles the emulator's sources unchanged)."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import synth

from batch_variants import instance
from early_host import pyearly
from test_packed_resident_gpu import _switched_ladder

STEPS = 64


def _chain(n):
    flat, dt, steps, src = synth.chain_batch("diode_chain", n, [3], tran=".tran 1e-6 7e-5")
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


def _switched_one():
    flat, dt, src = _switched_ladder()
    return instance(flat, 2), dt, src


CASES = {
    "diode_chain_100": lambda: _chain(100),    # 99 elements of a kind on 512 threads: most record slots are zero fill
    "diode_chain_1000": lambda: _chain(1000),  # the bench circuit: both items of (almost) every thread exist
    "switched_ladder": _switched_one,          # B runs again within a step: the parked source value must survive it
}
_OFF: dict = {}


def _off_run(case):
    """The build without the record: computed once per case, never modified."""
    if case not in _OFF:
        flat, dt, src = CASES[case]()
        r = pyearly.run(flat, STEPS, dt, src, "off")
        assert r["status"] == 0 and r["fresh_fill"] == 1 and r["zpar_doubles"] == 0
        for a in (r["out_v"], r["out_i"], r["iters"], *r["state"].values()):
            a.setflags(write=False)
        _OFF[case] = (flat, dt, src, r)
    return _OFF[case]


@pytest.mark.parametrize("nan_fill", [False, True], ids=["zeroed", "nan_arena"])
@pytest.mark.parametrize("mode", ["record", "record_idle_waves"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_record_gives_the_bits_of_the_separate_loads(case, mode, nan_fill):
    flat, dt, src, ref = _off_run(case)
    got = pyearly.run(flat, STEPS, dt, src, mode, nan_fill=nan_fill)
    assert got["status"] == 0 and got["fresh_fill"] == 1
    # the record as the handle sizes it, every slot written by the prologue (a slot left NaN was never filled)
    assert got["zpar_doubles"] == flat.n_inst * 2 * 512 * 5 and got["zpar_left_nan"] == 0
    assert got["pcr_n"] > 0 and got["nV"] >= 1  # (a tridiagonal top: the idle-wave form rides on it; a source value to park)
    assert np.isfinite(got["out_v"]).all() and np.isfinite(got["out_i"]).all()
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(got[k], ref[k]), (case, k)
    for k, v in ref["state"].items():
        assert np.array_equal(got["state"][k], v), (case, k)
    if case == "switched_ladder":
        assert got["nS"] > 0 and int(got["iters"].max()) > 1


@pytest.mark.parametrize("mode", ["record", "record_idle_waves"])
def test_thread_order_within_a_phase_does_not_matter(mode):
    flat, dt, src, ref = _off_run("diode_chain_100")
    got = pyearly.run(flat, STEPS, dt, src, mode, reverse=True, nan_fill=True)
    assert got["status"] == 0
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(got[k], ref[k]), k


def test_plan_takes_the_early_build_for_the_fresh_shape_and_the_knob_keeps_the_plain_one(monkeypatch):
    flat, _, _ = _chain(1000)
    flat = flat.replicate(3)
    monkeypatch.delenv("SPICEY_NO_EARLY_PREFETCH", raising=False)
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL", raising=False)
    on = pyearly.plan(flat, geometry=2)
    assert on["rc"] == 0 and (on["packed"], on["fresh"], on["early"], on["threads"]) == (1, 1, 1, 512)
    assert on["zpar_doubles"] == 3 * 2 * 512 * 5
    monkeypatch.setenv("SPICEY_NO_EARLY_PREFETCH", "1")
    off = pyearly.plan(flat, geometry=2)
    assert off["rc"] == 0 and (off["packed"], off["fresh"], off["early"]) == (1, 1, 0) and off["zpar_doubles"] == 0
    assert off["shape"] == on["shape"]  # the same shape, its plain kernel
    # a shape without early-prefetch kernels never gets a record: the 6-entry packed build, the latency geometry
    monkeypatch.delenv("SPICEY_NO_EARLY_PREFETCH")
    monkeypatch.setenv("SPICEY_NO_FRESH_FILL", "1")
    plain = pyearly.plan(flat, geometry=2)
    assert plain["rc"] == 0 and (plain["packed"], plain["fresh"], plain["early"], plain["zpar_doubles"]) == (1, 0, 0, 0)
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL")
    lat = pyearly.plan(flat, geometry=1)
    assert lat["rc"] == 0 and (lat["packed"], lat["early"], lat["zpar_doubles"]) == (0, 0, 0)
