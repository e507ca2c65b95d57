"""The stamp fuse (tran_v2_run.h: SF — Z stamps the next step's matrix and right-hand side from registers, no phase B in the
time loop) on the CPU: the plan's predicate, the table the host deals for it, and the host form of the fused phases against
the host executor that stamps in phase B — the same bits in voltages, currents, iteration counts, solve count, status and
end state, also from an arena and a parameter record that start as NaN and with the threads of every phase in reverse
order (which is what shows a missing barrier between the two halves of Z on the CPU).

Chains (found with tests/stamp_fuse_host for n = 20 .. 1025): the plan takes the fuse for diode_chain(511 .. 1022) — wherever
it folds the last factor level into the top; 511 is the smallest, 1022 the largest.  The table builder by itself also
accepts shorter chains (it asks nothing of the top); the plan does not, for want of the fold.  On diode_chain(1000), the
bench circuit: 1001 stamped entries, 999 of them with the conductance of one diode, and 1001 rows, 999 with the companion
currents of capacitor k and diode k, one with the source's value, one with nothing; the free slots that take the two
static entries and the empty row are item 1 of threads 487 .. 511.

The harness is tests/stamp_fuse_host (it compiles the emulator's sources unchanged); `make asan` there builds and runs the
same code as a stand-alone program under the address and undefined-behaviour sanitizers (not part of the suite)."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist

from test_packed_resident_gpu import _switched_ladder
from stamp_fuse_host import pysf

STEPS = 8
T = 512
KNOB = "SPICEY_NO_STAMP_FUSE"
KNOBS = (KNOB, "SPICEY_NO_TOP_FOLD", "SPICEY_NO_U0_RESIDENT", "SPICEY_NO_TOP_REGS", "SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS",
         "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL", "SPICEY_FRESH_FILL_LINEAR")
SMALLEST, LARGEST = 511, 1022
TRAN = ".tran 1e-6 7e-5"


def _chain(n, seeds=(3,), kind="diode_chain"):
    flat, dt, steps, src = synth.chain_batch(kind, n, list(seeds), tran=TRAN)
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


def _from_text(text, steps=STEPS):
    ckt = parseNetlist(text)
    dt, total = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    assert total >= steps
    return abi.flatten(ckt), dt, abi.source_table(ckt, dt, total)[: steps + 1]


def edited_chain(n, old_prefix, new_line, steps=STEPS):
    """diode_chain(n) with the one line that starts with `old_prefix` replaced"""
    lines = synth.diode_chain(n, seed=3, tran=TRAN).split("\n")
    hit = [i for i, s in enumerate(lines) if s.startswith(old_prefix)]
    assert len(hit) == 1
    lines[hit[0]] = new_line
    return _from_text("\n".join(lines), steps)


def chain_with_inductor(n=1000, steps=STEPS):
    return edited_chain(n, "R500 ", "L500 n500 n501 1e-6", steps)


def chain_with_floating_diode(n=1000, steps=STEPS):
    return edited_chain(n, "D500 ", "D500 n500 n501 DM", steps)


def chain_with_bare_node(n=1000, cut=2, instances=3, steps=STEPS):
    """diode_chain(n) without D{cut} and C{cut}: node cut + 1 holds two resistors and nothing else, so its diagonal is a static
    stamped entry — and with both resistors at 1e16 ohm in instance 1 a pivot of 2e-16, below the 1e-15 of the reference,
    in the matrix of step 0.  The plan takes the fuse: the two elements leave together, diode i and capacitor i still meet."""
    lines = [s for s in synth.diode_chain(n, seed=3, tran=TRAN).split("\n") if not s.startswith((f"D{cut} ", f"C{cut} "))]
    flat, dt, src = _from_text("\n".join(lines), steps)
    flat = flat.replicate(instances)
    node = cut + 1
    assert node not in set(flat.D_np) | set(flat.C_n1)
    flat.R_val[1, (flat.R_n1 == node) | (flat.R_n2 == node)] = 1e16
    return flat, dt, src


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _fields_of_entry(dd):
    """[(diode, negative)] in the order of the descriptor's fields (program.h: ent_dd)"""
    out = []
    for f in (dd & 0x7FFF, (dd >> 15) & 0x7FFF):
        if f:
            out.append(((f & 0x3FFF) - 1, bool(f & 0x4000)))
    return out


def _fields_of_row(d0, d1, n_c, n_v, n_d):
    """[(kind, index, negative)] in the order of the descriptor's fields (program.h: row_desc); nL = 0"""
    out = []
    for f in (d0 & 0xFFFF, d0 >> 16, d1 & 0xFFFF, d1 >> 16):
        if f:
            ix = (f & 0x7FFF) - 1
            kind = ("C", ix) if ix < n_c else ("V", ix - n_c) if ix < n_c + n_v else ("D", ix - n_c - n_v)
            assert kind[0] != "D" or kind[1] < n_d
            out.append((*kind, bool(f & 0x8000)))
    return out


@pytest.mark.parametrize("n", [SMALLEST, 766, 1000, LARGEST])
def test_the_plan_takes_the_fuse_and_the_table_deals_every_sum_to_its_operands_thread(n, no_knobs):
    flat, dt, src = _chain(n)
    p = pysf.plan(flat, steps=STEPS, geometry=2)
    assert (p["rc"], p["stamp_fuse"], p["stamp_fuse_run"], p["top_fold"], p["top_fold_run"], p["packed"], p["fresh"], p["threads"]) == (0, 1, 1, 1, 1, 1, 1, T), p
    assert p["zpar_doubles"] == flat.n_inst * 2 * T * 5  # (the record itself: the tables behind it are the handle's business)
    assert pysf.plan(flat, steps=2**32 - 1, geometry=2)["stamp_fuse_run"] == 0  # (beyond the ready-argument kernel's step range)
    t = pysf.table(flat)
    assert t["ok"] == 1 and t["fold_ok"] == 1 and (t["n_keep"], t["n"], t["n_v"]) == (n + 1, n + 1, 1) and t["n_dyn_ent"] == n - 1
    tb = t["table"].astype(np.int64)
    ent, row, srcw = tb[:, 0:2], tb[:, 2:4], tb[:, 4]
    assert (tb[:, 5] == pysf.NONE).all()
    # every stamped entry exactly once (an entry's id is its index in W), every row exactly once (the source's in its thread's fifth word)
    have_e, have_r = ent[(ent & pysf.NONE) == 0], row[(row & pysf.NONE) == 0]
    assert sorted((have_e & 0xFFFF).tolist()) == list(range(t["n_keep"]))
    have_s = srcw[(srcw & pysf.NONE) == 0]
    assert np.nonzero((srcw & pysf.NONE) == 0)[0].tolist() == list(range(t["n_v"]))
    assert sorted((have_r & 0xFFFF).tolist() + (have_s & 0xFFFF).tolist()) == [t["xoff"] + r for r in range(t["n"])]
    # slot limits: two entries and two rows per thread is the table's shape; nothing else is set in a word
    flags = pysf.NONE | pysf.RECIP | pysf.F0 | pysf.F0_NEG | pysf.F1 | pysf.F1_NEG | pysf.SWAP | 0xFFFF
    assert not (tb[:, :5] & ~flags).any() and not (ent & pysf.SWAP).any() and not (row & pysf.RECIP).any()
    # ownership and field order: slot j of thread t draws on diode / capacitor t + j T only, in the descriptor's order
    dd, rd = t["ent_dd"].astype(np.int64), t["row_desc"].astype(np.int64)
    n_dyn = 0
    for tid in range(T):
        for j in range(2):
            w = int(ent[tid, j])
            if not w & pysf.NONE:
                d = int(dd[w & 0xFFFF])
                want = _fields_of_entry(d)
                got = [(tid + j * T, bool(w & neg)) for has, neg in ((pysf.F0, pysf.F0_NEG), (pysf.F1, pysf.F1_NEG)) if w & has]
                # (a descriptor's first field may be empty and its second not: the order of those present is what counts)
                assert got == want and bool(w & pysf.RECIP) == bool(d & (1 << 30)) and not d >> 31, (tid, j, hex(w), hex(d))
                n_dyn += bool(want)
            w = int(row[tid, j])
            if not w & pysf.NONE:
                r = (w & 0xFFFF) - t["xoff"]
                want = _fields_of_row(int(rd[r, 0]), int(rd[r, 1]), t["n_c"], t["n_v"], t["n_d"])
                cap = [("C", tid + j * T, bool(w & pysf.F0_NEG))] if w & pysf.F0 else []
                dio = [("D", tid + j * T, bool(w & pysf.F1_NEG))] if w & pysf.F1 else []
                assert (dio + cap if w & pysf.SWAP else cap + dio) == want, (tid, j, hex(w), want)
    assert n_dyn == t["n_dyn_ent"]
    for s in range(t["n_v"]):
        r = (int(srcw[s]) & 0xFFFF) - t["xoff"]
        assert _fields_of_row(int(rd[r, 0]), int(rd[r, 1]), t["n_c"], t["n_v"], t["n_d"]) == [("V", s, False)]
    if n == 1000:  # what depends on nothing sits in the free slots: item 1 of threads 487 .. 511
        free = [(tid, j) for tid in range(T) for j in range(2) if not ent[tid, j] & pysf.NONE and not ent[tid, j] & (pysf.F0 | pysf.F1)]
        assert free == [(487, 1), (488, 1)]
        assert [(tid, j) for tid in range(T) for j in range(2) if not row[tid, j] & pysf.NONE and not row[tid, j] & (pysf.F0 | pysf.F1)] == [(487, 1)]


def test_which_chains_take_the_fuse(no_knobs):
    takes = {n: pysf.plan(_chain(n)[0], steps=STEPS, geometry=2)["stamp_fuse_run"] for n in (100, 510, SMALLEST, LARGEST, 1023)}
    assert takes == {100: 0, 510: 0, SMALLEST: 1, LARGEST: 1, 1023: 0}


REFUSALS = {
    "rc_ladder": lambda: _chain(1000, kind="rc_ladder"),  # linear: a reused factorisation stamps nothing
    "switched_ladder": lambda: (lambda f, dt, s: (f, dt, s[: STEPS + 1]))(*_switched_ladder()),  # nS > 0: the step re-iterates
    "inductor": chain_with_inductor,
    "rcd_mesh": lambda: _from_text(synth.rcd_mesh(12, tran=TRAN)),
    "floating_diode": chain_with_floating_diode,  # one diode stamps four entries: one slot cannot hold them
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_plan_refuses_the_fuse_where_its_conditions_fail(case, no_knobs):
    flat, dt, src = REFUSALS[case]()
    p = pysf.plan(flat, steps=STEPS, geometry=2)
    assert (p["rc"], p["stamp_fuse"], p["stamp_fuse_run"]) == (0, 0, 0), p
    assert pysf.table(flat)["ok"] <= 0
    if case == "switched_ladder":
        assert p["top_fold"] == 1 and flat.nS > 0  # (today's form stays)
    # the harness refuses too, and the form a plan without the fuse takes runs
    assert pysf.run(flat, 2, dt, src[:3], fuse=True)["status"] != 0
    if case != "rcd_mesh":  # (a mesh has no tridiagonal top: none of the harness's builds is the plan's)
        assert pysf.run(flat, 2, dt, src[:3], fuse=False)["status"] == 0


def test_the_knob_and_a_plan_without_the_fold_keep_todays_form(no_knobs):
    flat, dt, src = _chain(1000)
    assert pysf.plan(flat, steps=STEPS, geometry=2)["stamp_fuse"] == 1
    no_knobs.setenv(KNOB, "1")
    p = pysf.plan(flat, steps=STEPS, geometry=2)
    assert (p["rc"], p["stamp_fuse"], p["stamp_fuse_run"], p["top_fold"], p["top_fold_run"]) == (0, 0, 0, 1, 1)
    no_knobs.delenv(KNOB)
    for knob in ("SPICEY_NO_TOP_FOLD", "SPICEY_NO_U0_RESIDENT", "SPICEY_NO_TOP_REGS"):
        no_knobs.setenv(knob, "1")
        p = pysf.plan(flat, steps=STEPS, geometry=2)
        assert (p["rc"], p["stamp_fuse"], p["stamp_fuse_run"], p["top_fold"], p["packed"]) == (0, 0, 0, 0, 1), knob
        no_knobs.delenv(knob)
    p = pysf.plan(flat, steps=STEPS, geometry=1)  # the latency geometry has no such kernel
    assert (p["rc"], p["stamp_fuse"], p["packed"]) == (0, 0, 0)


def _same(got, ref, what):
    for k in ("out_v", "out_i", "iters"):
        if ref[k] is not None:
            assert got[k].tobytes() == ref[k].tobytes(), (what, k)
    for k, v in ref["state"].items():
        assert np.asarray(got["state"][k]).tobytes() == np.asarray(v).tobytes(), (what, k)
    assert got["solves"] == ref["solves"] and got["status"] == ref["status"] and np.array_equal(got["err4"], ref["err4"]), what


_CASES = {"diode_chain_511": lambda: _chain(SMALLEST, seeds=(3, 4)), "diode_chain_1000": lambda: _chain(1000, seeds=(3, 4)), "diode_chain_1022": lambda: _chain(LARGEST)}
_REF: dict = {}


def _ref(case):
    """The unfused host executor, run once per case: a first run and a second one from the first one's end state"""
    if case not in _REF:
        flat, dt, src = _CASES[case]()
        r1 = pysf.run(flat, STEPS, dt, src, fuse=False)
        r2 = pysf.run(flat, STEPS, dt, src, fuse=False, state=r1["state"])
        for r in (r1, r2):
            assert r["status"] == 0 and r["table_ok"] == 1 and r["fold_ok"] == 1
            for a in (r["out_v"], r["out_i"], r["iters"], *r["state"].values()):
                a.setflags(write=False)
        _REF[case] = (flat, dt, src, r1, r2)
    return _REF[case]


@pytest.mark.parametrize("variant", ["zeroed", "nan_arena_reversed"])
@pytest.mark.parametrize("case", sorted(_CASES))
def test_the_fused_phases_give_the_bits_of_the_executor_with_phase_b(case, variant, no_knobs):
    flat, dt, src, ref, ref2 = _ref(case)
    odd = variant != "zeroed"
    got = pysf.run(flat, STEPS, dt, src, fuse=True, nan_fill=odd, reverse=odd)
    assert got["status"] == 0
    assert np.isfinite(got["out_v"]).all() and np.isfinite(got["out_i"]).all() and float(np.abs(got["out_v"]).max()) > 1.0
    _same(got, ref, (case, variant))
    # a second run on the same state: the prologue stamps from what the first one left
    again = pysf.run(flat, STEPS, dt, src, fuse=True, nan_fill=odd, reverse=odd, state=got["state"])
    _same(again, ref2, (case, variant, "second run"))
    assert not np.array_equal(again["out_v"], got["out_v"])


@pytest.mark.parametrize("variant", ["one_step", "no_currents"])
def test_run_edges(variant, no_knobs):
    flat, dt, src = _chain(1000, seeds=(3, 4))
    steps = 1 if variant == "one_step" else STEPS
    kw = dict(currents=variant != "no_currents")
    ref = pysf.run(flat, steps, dt, src[: steps + 1], fuse=False, **kw)
    got = pysf.run(flat, steps, dt, src[: steps + 1], fuse=True, nan_fill=True, reverse=True, **kw)
    assert ref["status"] == 0 and got["status"] == 0 and (got["out_i"] is None) == (variant == "no_currents")
    _same(got, ref, variant)
    zero = pysf.run(flat, 0, dt, src[:1], fuse=True, nan_fill=True, reverse=True, **kw)  # the prologue's stamps alone, nothing fused runs
    _same(zero, pysf.run(flat, 0, dt, src[:1], fuse=False, **kw), (variant, "no step"))


def test_a_singular_pivot_in_the_stamps_of_step_0_ends_the_run_as_phase_b_ended_it(no_knobs):
    """The fused form stamps step 0 in its prologue: a pivot below the bar found there must give the status, instance, error
    step, iteration, recorded outputs and state of today's failure in step 0."""
    flat, dt, src = chain_with_bare_node()
    per = np.ascontiguousarray(np.broadcast_to(src, (3, STEPS + 1, flat.nV)))
    assert pysf.plan(flat, steps=STEPS, geometry=2)["stamp_fuse_run"] == 1
    ref = pysf.run(flat, STEPS, dt, per, fuse=False)
    got = pysf.run(flat, STEPS, dt, per, fuse=True, nan_fill=True, reverse=True)
    assert ref["status"] == abi.ERR_SINGULAR and ref["err4"].tolist() == [1, 1, 0, 0]
    _same(got, ref, "bare node")
    assert not got["iters"][1].any() and got["iters"][0].all() and got["iters"][2].all()
