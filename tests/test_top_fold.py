"""The fold of the last factor level into the tridiagonal top (tran_v2_run.h: TF) on the CPU: the plan's predicate, the
record table the host builds for it, and the host restatement of the folded top (spicey_top_fold_wave: "record, then the
stages", the lane exchange as array indexing) against the unfolded host executor — the same bits in voltages, currents,
iteration counts, solve count, status and end state, also from an arena and a parameter record that start as NaN and with
the threads of every phase in reverse order.

Chains (found with tests/top_fold_host for n = 20 .. 1023): the plan takes the fold for diode_chain(511 .. 1022) — wherever
it takes the resident level-0 record — and diode_chain(511) is the smallest: a top of 33 rows, four of them with a single
pivot, row 0 among them.  diode_chain(766) has a top of 63 rows (the program has no row-record encoding of the level there:
the table is built from the level's task records), diode_chain(1000) — the bench circuit — 64 rows, rows 0 and 1 with a
single pivot; where the program has row records for the level, the table's records are those records field for field, but
for the targets they create.

The harness is tests/top_fold_host (it compiles the emulator's sources unchanged); `make asan` there builds and runs the
same code as a stand-alone program under the address and undefined-behaviour sanitizers (not part of the suite)."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist

from batch_variants import instance
from test_packed_resident_gpu import _switched_ladder
from top_fold_host import pytf

STEPS = 8
T = 512
KNOB = "SPICEY_NO_TOP_FOLD"
KNOBS = (KNOB, "SPICEY_NO_U0_RESIDENT", "SPICEY_NO_TOP_REGS", "SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH",
         "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL", "SPICEY_FRESH_FILL_LINEAR")
VALID, RECIP, FUSED = 0x8000, 0x0200, 0x0400  # (meta half-word of a row record: program.h)


def _chain(n, seeds=(3,), kind="diode_chain"):
    flat, dt, steps, src = synth.chain_batch(kind, n, list(seeds), tran=".tran 1e-6 7e-5")
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


def _mesh():
    ckt = parseNetlist(synth.rcd_mesh(12, tran=".tran 1e-6 7e-5"))
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    return abi.flatten(ckt), dt, abi.source_table(ckt, dt, steps)[: STEPS + 1]


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# chain length -> (rows of the top, rows with a single pivot)
CHAINS = {511: (33, [0, 1, 22, 23]), 766: (63, []), 1000: (64, [0, 1])}


@pytest.mark.parametrize("n", sorted(CHAINS))
def test_the_plan_takes_the_fold_and_the_table_is_the_levels_records(n, no_knobs):
    rows, single = CHAINS[n]
    flat, dt, src = _chain(n)
    p = pytf.plan(flat, steps=STEPS, geometry=2)
    assert (p["rc"], p["top_fold"], p["top_fold_run"], p["u0_resident_run"], p["packed"], p["fresh"], p["threads"], p["pcr_n"]) == (0, 1, 1, 1, 1, 1, T, rows), p
    assert p["pcr_level"] >= 1
    assert pytf.plan(flat, steps=2**32 - 1, geometry=2)["top_fold_run"] == 0  # (beyond the ready-argument kernel's step range)
    t = pytf.table(flat)
    assert t["ok"] == 1 and t["pcr_n"] == rows
    tb, tab, zs = t["table"].astype(np.int64), t["tab"].astype(np.int64), t["zero_slot"]
    meta = tb[:rows, 1]
    piv, o0, o1 = meta & 3, (meta >> 4) & 1, (meta >> 5) & 1
    assert ((meta & VALID) != 0).all() and ((meta & RECIP) == 0).all() and (piv >= 1).all()
    assert np.nonzero(piv == 1)[0].tolist() == single
    assert not tb[rows:].any()  # lanes past the top: no record
    # the four targets are the row's own entries of the top's index table (a created one: the +0.0 slot)
    new_aii, new0, new1 = (meta & 0x04) != 0, (meta & 0x40) != 0, (meta & 0x80) != 0
    assert (tb[:rows, 0] == np.where(new_aii, zs, tab[:rows, 1])).all() and (tb[:rows, 2] == tab[:rows, 3]).all()
    sup0 = tb[:rows, 15] == 1
    assert set(tb[:rows, 15].tolist()) <= {0, 1}
    side0, side1 = np.where(sup0, tab[:rows, 2], tab[:rows, 0]), np.where(sup0, tab[:rows, 0], tab[:rows, 2])
    for side, field, has, new in ((side0, 8, o0 == 1, new0), (side1, 14, (o1 == 1) & (piv == 2), new1)):
        want = np.where(has & new, zs, np.where(side == 0xFFFF, zs, side))
        assert (tb[:rows, field] == want).all()
        assert not (has & (side == 0xFFFF)).any()  # a fill has a neighbour to go to
    assert (0 < zs < 0xFFFF) and len(set(tab[:rows, 1].tolist())) == rows
    # where the program has a row-record encoding of the level, these ARE its records (but for the created targets)
    if t["row_records"]:
        assert t["row_records"] == rows and t["remainder"] == 0
        by_diag = {int(r[0]): r for r in t["rows"][:rows].astype(np.int64)}
        for i in range(rows):
            r = by_diag[int(tab[i, 1])]
            assert tb[i, 1] == r[1] and (tb[i, 2:8] == r[2:8]).all() and (tb[i, 9:14] == r[9:14]).all(), i
            assert tb[i, 0] == (zs if r[1] & 0x04 else r[0])
            if r[1] & 0x10: assert tb[i, 8] == (zs if r[1] & 0x40 else r[8])
            if (r[1] & 0x20) and (r[1] & 3) == 2: assert tb[i, 14] == (zs if r[1] & 0x80 else r[14])
    else:
        assert rows < 64  # (the program encodes a level as row records from 64 rows on)
    assert (t["row_records"] != 0) == (n == 1000)


def test_the_plan_refuses_the_fold_where_its_conditions_fail(no_knobs):
    flat, dt, src = _chain(1000)
    assert pytf.plan(flat, steps=STEPS, geometry=2)["top_fold"] == 1
    # the knob: the resident-record kernel stays
    no_knobs.setenv(KNOB, "1")
    p = pytf.plan(flat, steps=STEPS, geometry=2)
    assert (p["rc"], p["top_fold"], p["top_fold_run"], p["u0_resident"], p["u0_resident_run"]) == (0, 0, 0, 1, 1)
    no_knobs.delenv(KNOB)
    # a plan without the register-exchange top, or without the resident record, has no such form
    for knob in ("SPICEY_NO_TOP_REGS", "SPICEY_NO_U0_RESIDENT"):
        no_knobs.setenv(knob, "1")
        p = pytf.plan(flat, steps=STEPS, geometry=2)
        assert (p["rc"], p["top_fold"], p["top_fold_run"], p["packed"]) == (0, 0, 0, 1), knob
        no_knobs.delenv(knob)
    # the latency geometry has no such kernel
    p = pytf.plan(flat, steps=STEPS, geometry=1)
    assert (p["rc"], p["top_fold"], p["packed"]) == (0, 0, 0)
    # a linear circuit reuses its factors: the right-hand-side column of the level alone is no record of the table
    lin = _chain(1000, kind="rc_ladder")[0]
    p = pytf.plan(lin, steps=STEPS, geometry=2)
    assert (p["rc"], p["top_fold"], p["top_fold_run"], p["packed"]) == (0, 0, 0, 1)
    assert pytf.table(lin)["ok"] <= 0
    # a mesh: no tridiagonal top, generic tasks everywhere
    mesh = _mesh()[0]
    p = pytf.plan(mesh, steps=STEPS, geometry=2)
    assert (p["rc"], p["top_fold"], p["top_fold_run"], p["pcr_n"]) == (0, 0, 0, 0)
    # chains whose level 0 stays in the slots (no resident record) and the longest one (a record more than threads)
    for n in (22, 100, 510, 1023):
        p = pytf.plan(_chain(n)[0], steps=STEPS, geometry=2)
        assert (p["rc"], p["top_fold"], p["u0_resident"]) == (0, 0, 0), n


def _same(got, ref, what):
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    for k, v in ref["state"].items():
        assert np.array_equal(got["state"][k], v), (what, k)
    assert got["solves"] == ref["solves"] and got["status"] == ref["status"] and np.array_equal(got["err4"], ref["err4"]), what


_CASES = {
    "diode_chain_511": lambda: _chain(511, seeds=(3, 4)),
    "diode_chain_1000": lambda: _chain(1000, seeds=(3, 4)),
    "switched_ladder": lambda: (lambda f, dt, s: (instance(f, 2), dt, s[: STEPS + 1]))(*_switched_ladder()),
}
_REF: dict = {}


def _ref(case):
    if case not in _REF:
        flat, dt, src = _CASES[case]()
        r = pytf.run(flat, STEPS, dt, src, fold=False)
        assert r["status"] == 0 and r["table_ok"] == 1 and r["u0_fits"] == 1
        for a in (r["out_v"], r["out_i"], r["iters"], *r["state"].values()):
            a.setflags(write=False)
        _REF[case] = (flat, dt, src, r)
    return _REF[case]


@pytest.mark.parametrize("variant", ["zeroed", "nan_arena_reversed"])
@pytest.mark.parametrize("case", sorted(_CASES))
def test_the_folded_top_gives_the_bits_of_the_unfolded_executor(case, variant, no_knobs):
    flat, dt, src, ref = _ref(case)
    got = pytf.run(flat, STEPS, dt, src, fold=True, nan_fill=variant != "zeroed", reverse=variant != "zeroed")
    assert got["status"] == 0 and got["with_pivot"] >= 1
    assert np.isfinite(got["out_v"]).all() and np.isfinite(got["out_i"]).all() and float(np.abs(got["out_v"]).max()) > 1.0
    _same(got, ref, (case, variant))
    if case == "switched_ladder":
        assert flat.nS > 0 and int(got["iters"].max()) > 1


def test_the_harness_refuses_the_fold_where_the_plan_would(no_knobs):
    for n in (100, 1023):
        flat, dt, src = _chain(n)
        assert pytf.run(flat, 2, dt, src[:3], fold=True)["status"] != 0
        assert pytf.run(flat, 2, dt, src[:3], fold=False)["status"] == 0
