"""The fixed schedule (tran_v2_run.h: FS — the time loop of the fused packed build written out for what the plan holds: no
phase masks, no streamed path, no overflow list, no fork on the phase table, the iteration counts written once behind the
loop) on the CPU: the plan's predicate and its refusals, and the host form of the written-out loop against the host form of
the loop that decides its schedule in every step — the same bits in voltages, currents, iteration counts, solve count,
status and end state, also from an arena and a parameter record that start as NaN, with the threads of every phase in
reverse order, and on an executor without idle waves (the early fetch in a phase of its own).

Chains (found with tests/fixed_schedule_host): the plan takes the form for diode_chain(511 .. 638) and (896 .. 1018).  The
fuse itself is taken for 511 .. 1022; in 639 .. 895 and 1019 .. 1022 the resident layout streams a second phase beside
level 0 (the slots do not hold every level), which the written-out loop has no path for: the predicate refuses, and the
fused kernel of today runs.  diode_chain(1000), the bench circuit, takes the form.

The harness is tests/fixed_schedule_host (it compiles the emulator's sources unchanged); `make asan` there builds and runs
the same code as a stand-alone program under the address and undefined-behaviour sanitizers (not part of the suite)."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import abi, synth

from test_packed_resident_gpu import _switched_ladder
from test_stamp_fuse import chain_with_inductor, _from_text
from test_top_regs_gpu import _half_clamped_chain
from fixed_schedule_host import pyfs

STEPS = 8
T = 512
KNOB = "SPICEY_NO_FIXED_SCHEDULE"
KNOBS = (KNOB, "SPICEY_NO_STAMP_FUSE", "SPICEY_NO_TOP_FOLD", "SPICEY_NO_U0_RESIDENT", "SPICEY_NO_TOP_REGS", "SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS",
         "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL", "SPICEY_FRESH_FILL_LINEAR", "SPICEY_NO_KMERGE")
TAKEN = (511, 638, 896, 1000, 1018)          # the ends of the two ranges, and the bench circuit
FUSED_ONLY = (639, 766, 895, 1019, 1022)     # the fuse, but a second streamed phase
TRAN = ".tran 1e-6 7e-5"


def _chain(n, seeds=(3,), kind="diode_chain", steps=STEPS):
    flat, dt, total, src = synth.chain_batch(kind, n, list(seeds), tran=TRAN)
    assert total >= steps
    return flat, dt, src[: steps + 1]


def singular_later(steps=64):
    """diode_chain(1000) x 3 whose instance 1 has nodes 500 and 501 tied by 2^-20 ohm and cut off from the chain (1e16 ohm), their
    capacitors at 1e-24 F and their diodes started at 0.6 V: the pair discharges through the diodes by one thermal voltage a
    step, and once a diode's conductance falls below half an ulp of the 2^20 S between the nodes both diagonals are 2^20
    exactly, the multiplier is 1 exactly (a power of two: its reciprocal is exact on every device) and the second pivot of
    the pair is 0 — some 17 steps in.  Only values differ from the plain chain: the plan is the same."""
    flat, dt, total, src = synth.chain_batch("diode_chain", 1000, [3], tran=TRAN)
    assert total >= steps
    flat = flat.replicate(3)
    a, b = 500, 501
    inner = ((flat.R_n1 == a) & (flat.R_n2 == b)) | ((flat.R_n1 == b) & (flat.R_n2 == a))
    outer = ((flat.R_n1 == a) | (flat.R_n2 == a) | (flat.R_n1 == b) | (flat.R_n2 == b)) & ~inner
    dio, cap = (flat.D_np == a) | (flat.D_np == b), (flat.C_n1 == a) | (flat.C_n1 == b)
    assert (inner.sum(), outer.sum(), dio.sum(), cap.sum()) == (1, 2, 2, 2)
    flat.R_val[1, inner] = 2.0 ** -20
    flat.R_val[1, outer] = 1e16
    flat.C_val[1, cap] = 1e-24
    flat.D_vdprev[1, dio] = 0.6
    return flat, dt, np.ascontiguousarray(np.broadcast_to(src[: steps + 1], (3, steps + 1, flat.nV)))


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _plan(flat, steps=STEPS, **options):
    options.setdefault("geometry", 2)
    return pyfs.plan(flat, steps=steps, **options)


def test_which_chains_take_the_form(no_knobs):
    got = {n: (lambda p: (p["rc"], p["fixed_schedule"], p["fixed_schedule_run"], p["stamp_fuse_run"]))(_plan(_chain(n)[0])) for n in (510,) + TAKEN + FUSED_ONLY + (1023,)}
    want = {510: (0, 0, 0, 0), 1023: (0, 0, 0, 0), **{n: (0, 1, 1, 1) for n in TAKEN}, **{n: (0, 0, 0, 1) for n in FUSED_ONLY}}
    assert got == want
    p = _plan(_chain(1000)[0])
    assert (p["packed"], p["fresh"], p["threads"], p["top_fold"]) == (1, 1, T, 1)
    assert _plan(_chain(1000)[0], steps=2**32 - 1)["fixed_schedule_run"] == 0  # (beyond the ready-argument kernel's step range)


@pytest.mark.parametrize("n", [511, 1000, 1018])
def test_the_predicate_refuses_every_layout_the_written_out_loop_cannot_run(n, no_knobs):
    p = pyfs.predicate(_chain(n)[0])
    assert p == {"rc": 0, "as_built": 1, "streamed_backward_phase": 0, "unmerged": 0, "three_products": 0, "empty_factor_phase": 0, "lds_tail": 0, "top_of_65_rows": 0}


@pytest.mark.parametrize("n", FUSED_ONLY)
def test_a_chain_with_a_second_streamed_phase_is_refused_and_keeps_the_fuse(n, no_knobs):
    flat, dt, src = _chain(n)
    r = pyfs.run(flat, 1, dt, src[:2], fixed=False)
    assert r["status"] == 0 and (r["fs_fits"], r["fuse_ok"], r["streamed_phases"]) == (0, 1, 2)
    assert pyfs.predicate(flat)["as_built"] == 0
    assert pyfs.run(flat, 1, dt, src[:2], fixed=True)["status"] == abi.ERR_BAD_DESC


REFUSALS = {
    "rc_ladder": lambda: _chain(1000, kind="rc_ladder"),  # linear: no fuse
    "switched_ladder": lambda: (lambda f, dt, s: (f, dt, s[: STEPS + 1]))(*_switched_ladder()),  # nS > 0: the step re-iterates
    "inductor": chain_with_inductor,
    "rcd_mesh": lambda: _from_text(synth.rcd_mesh(12, tran=TRAN)),  # no tridiagonal top
    "half_clamped_chain": lambda: (lambda f, dt, s: (f, dt, s[: STEPS + 1]))(*_half_clamped_chain(1000)),  # the chain of the fold's singular test: no fuse
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_plan_refuses_the_form_where_its_conditions_fail(case, no_knobs):
    flat, dt, src = REFUSALS[case]()
    p = _plan(flat)
    assert (p["rc"], p["fixed_schedule"], p["fixed_schedule_run"], p["stamp_fuse"]) == (0, 0, 0, 0), p
    assert pyfs.run(flat, 2, dt, src[:3], fixed=True)["status"] != 0  # the harness refuses too


def test_the_knob_the_empty_phases_and_a_plan_without_the_fuse_keep_todays_form(no_knobs):
    flat, dt, src = _chain(1000)
    assert _plan(flat)["fixed_schedule_run"] == 1
    no_knobs.setenv(KNOB, "1")
    p = _plan(flat)
    assert (p["rc"], p["fixed_schedule"], p["fixed_schedule_run"], p["stamp_fuse"], p["stamp_fuse_run"]) == (0, 0, 0, 1, 1)
    no_knobs.delenv(KNOB)
    # debug_empty_phases = 1 (SpiceyOptions.debug bits 8 and up): the written-out loop has no empty phases
    p = _plan(flat, debug=1 << 8)
    assert (p["rc"], p["fixed_schedule"], p["fixed_schedule_run"], p["stamp_fuse_run"]) == (0, 0, 0, 1)
    for knob in ("SPICEY_NO_STAMP_FUSE", "SPICEY_NO_TOP_FOLD", "SPICEY_NO_U0_RESIDENT", "SPICEY_NO_PHASE_TABLE"):
        no_knobs.setenv(knob, "1")
        p = _plan(flat)
        # (the plan's flag is a property of the program and its shape, like `stamp_fuse`: without the phase table it stands, and no run takes it)
        assert (p["rc"], p["fixed_schedule"], p["fixed_schedule_run"], p["stamp_fuse_run"], p["packed"]) == (0, int(knob == "SPICEY_NO_PHASE_TABLE"), 0, 0, 1), knob
        no_knobs.delenv(knob)
    # without the merged backward phase the layout is another one: refused, the fuse stays
    no_knobs.setenv("SPICEY_NO_KMERGE", "1")
    p = _plan(flat)
    assert (p["rc"], p["fixed_schedule_run"], p["stamp_fuse_run"]) == (0, 0, 1)
    no_knobs.delenv("SPICEY_NO_KMERGE")
    p = _plan(flat, geometry=1)  # the latency geometry has no such kernel
    assert (p["rc"], p["fixed_schedule"], p["packed"]) == (0, 0, 0)


def _same(got, ref, what):
    for k in ("out_v", "out_i", "iters"):
        if ref[k] is not None:
            assert got[k].tobytes() == ref[k].tobytes(), (what, k)
    for k, v in ref["state"].items():
        assert np.asarray(got["state"][k]).tobytes() == np.asarray(v).tobytes(), (what, k)
    assert got["solves"] == ref["solves"] and got["status"] == ref["status"] and np.array_equal(got["err4"], ref["err4"]), what


_CASES = {"diode_chain_511": lambda: _chain(511, seeds=(3, 4)), "diode_chain_1000": lambda: _chain(1000, seeds=(3, 4))}
_REF: dict = {}


def _ref(case):
    """The loop that decides its schedule in every step, run once per case: a first run and a second one from its end state"""
    if case not in _REF:
        flat, dt, src = _CASES[case]()
        r1 = pyfs.run(flat, STEPS, dt, src, fixed=False)
        r2 = pyfs.run(flat, STEPS, dt, src, fixed=False, state=r1["state"])
        for r in (r1, r2):
            assert r["status"] == 0 and r["fs_fits"] == 1
            for a in (r["out_v"], r["out_i"], r["iters"], *r["state"].values()):
                a.setflags(write=False)
        _REF[case] = (flat, dt, src, r1, r2)
    return _REF[case]


@pytest.mark.parametrize("variant", ["zeroed", "nan_arena_reversed", "no_idle_waves"])
@pytest.mark.parametrize("case", sorted(_CASES))
def test_the_written_out_loop_gives_the_bits_of_the_loop_that_decides_in_every_step(case, variant, no_knobs):
    flat, dt, src, ref, ref2 = _ref(case)
    kw = dict(nan_fill=variant != "zeroed", reverse=variant == "nan_arena_reversed", idle_waves=variant != "no_idle_waves")
    got = pyfs.run(flat, STEPS, dt, src, fixed=True, **kw)
    assert got["status"] == 0
    assert np.isfinite(got["out_v"]).all() and np.isfinite(got["out_i"]).all() and float(np.abs(got["out_v"]).max()) > 1.0
    assert (got["iters"] == 1).all()
    _same(got, ref, (case, variant))
    # a second run on the same state
    again = pyfs.run(flat, STEPS, dt, src, fixed=True, state=got["state"], **kw)
    _same(again, ref2, (case, variant, "second run"))
    assert not np.array_equal(again["out_v"], got["out_v"])


@pytest.mark.parametrize("variant", ["one_step", "no_currents", "no_step"])
def test_run_edges(variant, no_knobs):
    flat, dt, src = _chain(1000, seeds=(3, 4))
    steps = {"one_step": 1, "no_step": 0}.get(variant, STEPS)
    kw = dict(currents=variant != "no_currents")
    ref = pyfs.run(flat, steps, dt, src[: steps + 1], fixed=False, **kw)
    got = pyfs.run(flat, steps, dt, src[: steps + 1], fixed=True, nan_fill=True, reverse=True, iters_fill=-7, **kw)
    assert ref["status"] == 0 and got["status"] == 0 and (got["out_i"] is None) == (variant == "no_currents")
    assert (got["iters"] == 1).all() and got["iters"].shape == (2, steps + 1)
    _same(got, ref, variant)


def test_a_pivot_that_turns_singular_at_a_later_step_ends_the_run_the_same_way_and_leaves_the_counts_behind_it_alone(no_knobs):
    flat, dt, per = singular_later()
    assert _plan(flat, steps=64)["fixed_schedule_run"] == 1
    ref = pyfs.run(flat, 64, dt, per, fixed=False, iters_fill=-7)
    got = pyfs.run(flat, 64, dt, per, fixed=True, nan_fill=True, reverse=True, iters_fill=-7)
    assert ref["status"] == abi.ERR_SINGULAR and ref["err4"][0] == 1 and ref["err4"][1] == 1 and ref["err4"][3] == 0
    step = int(ref["err4"][2])
    assert 0 < step < 64
    _same(got, ref, "singular at a later step")
    assert (got["iters"][1][:step] == 1).all() and (got["iters"][1][step:] == -7).all()
    assert (got["iters"][0] == 1).all() and (got["iters"][2] == 1).all()
