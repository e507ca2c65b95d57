"""The resident level-0 record (tran_v2_run.h: UR) on the CPU: the packed layout (512 threads, 4 slots) of the fresh
operand-address build whose prologue loads the row record of factor level 0 into eight registers once, whose phase B
fetches nothing and whose phase 0 runs the registers — against the same build that fetches the record under B in every
step: same bits in voltages, currents, iteration counts, solve count, status and end state, also from an arena (and
record registers) that start as NaN / all ones and with the threads of every phase in reverse order.  Every run takes the
form the launch plan chooses for the circuit without SPICEY_NO_U0_RESIDENT, against the one it chooses with the knob.
diode_chain(22) (the smallest chain with a top) and diode_chain(100) keep level 0 resident in the slots, so no plan takes
the form there and both runs are the same kernel; diode_chain(1000) — the bench circuit — and the switched ladder take it.

Also: where the plan takes the form; the record words against the program's own; and the port of the device library's
exp (tran_common.h: spicey_exp_port) as the host compiles it against the host's exp — a smoke test of the port, the
bit-identity proof is tests/test_u0_resident_gpu.py.

The harness is tests/u0_host (it compiles the emulator's sources unchanged); `make asan` there builds and runs the same
code as a stand-alone program under the address and undefined-behaviour sanitizers (not part of the suite: a build of
two minutes)."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist

from batch_variants import instance
from test_packed_resident_gpu import _switched_ladder
from test_top_regs_gpu import _half_clamped_chain
from u0_host import pyu0

STEPS = 64
T = 512
KNOB = "SPICEY_NO_U0_RESIDENT"
KNOBS = (KNOB, "SPICEY_NO_TOP_REGS", "SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE",
         "SPICEY_NO_FRESH_FILL", "SPICEY_FRESH_FILL_LINEAR")


def _chain(n, seeds=(3,), kind="diode_chain"):
    flat, dt, steps, src = synth.chain_batch(kind, n, list(seeds), tran=".tran 1e-6 7e-5")
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


def _switched_one():
    flat, dt, src = _switched_ladder()
    return instance(flat, 2), dt, src


# case -> (circuit, whether the plan takes the form, row records of level 0 where it does)
CASES = {
    "diode_chain_22": (lambda: _chain(22), False, 0),       # the smallest chain with a top: level 0 is resident in the slots
    "diode_chain_100": (lambda: _chain(100), False, 0),
    "diode_chain_1000": (lambda: _chain(1000), True, 512),  # the bench circuit: a record in every thread
    "switched_ladder": (_switched_one, True, None),         # B and the solve run twice in a step, with a_reiterate between them
}
_REF: dict = {}


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _ref_run(case, monkeypatch):
    """The circuit, the form its plan takes, and the run of the build that fetches the record under B: computed once per
    case, never modified."""
    if case not in _REF:
        flat, dt, src = CASES[case][0]()
        on = pyu0.plan(flat, steps=STEPS, geometry=2)
        monkeypatch.setenv(KNOB, "1")
        off = pyu0.plan(flat, steps=STEPS, geometry=2)
        monkeypatch.delenv(KNOB)
        assert on["rc"] == 0 and off["rc"] == 0 and (off["u0_resident"], off["u0_resident_run"]) == (0, 0)
        assert (on["packed"], on["fresh"], on["threads"], on["inst_per_wg"], on["top_regs_run"]) == (1, 1, T, 1, 1)
        assert {k: v for k, v in off.items() if not k.startswith("u0_")} == {k: v for k, v in on.items() if not k.startswith("u0_")}
        r = pyu0.run(flat, STEPS, dt, src, resident=False)
        assert r["status"] == 0
        for a in (r["out_v"], r["out_i"], r["iters"], *r["state"].values()):
            a.setflags(write=False)
        _REF[case] = (flat, dt, src, on, r)
    return _REF[case]


def _same(got, ref, what):
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    for k, v in ref["state"].items():
        assert np.array_equal(got["state"][k], v), (what, k)
    assert got["solves"] == ref["solves"] and got["status"] == ref["status"] and np.array_equal(got["err4"], ref["err4"]), what


@pytest.mark.parametrize("variant", ["zeroed", "nan_arena", "reversed"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_resident_record_gives_the_bits_of_the_fetched_one(case, variant, no_knobs):
    flat, dt, src, plan, ref = _ref_run(case, no_knobs)
    takes, records = CASES[case][1], CASES[case][2]
    assert plan["u0_resident_run"] == int(takes) and plan["u0_resident"] == int(takes), plan
    got = pyu0.run(flat, STEPS, dt, src, resident=takes, nan_fill=variant != "zeroed", reverse=variant == "reversed")
    assert got["status"] == 0 and got["fits"] == int(takes) and got["pcr_n"] > 0
    if records is not None and takes:
        assert (got["rows"], got["records"], got["remainder"]) == (1, records, 0)
    assert np.isfinite(got["out_v"]).all() and np.isfinite(got["out_i"]).all()
    _same(got, ref, (case, variant))
    assert int(got["iters"].min()) >= 1
    if case == "switched_ladder":
        assert flat.nS > 0 and int(got["iters"].max()) > 1
    assert not np.array_equal(got["state"]["C_vprev"], flat.C_vprev)  # (the run did move the state)
    if not takes:  # the harness refuses the form where the plan would
        assert pyu0.run(flat, 2, dt, src[:3], resident=True)["status"] != 0


def test_where_the_plan_takes_the_form(no_knobs):
    # the bench circuit, and every chain whose level 0 is streamed as row records: fewer records than threads, T - 1, T
    for n, records in ((600, None), (766, T - 1), (893, T - 1), (894, T), (1000, T), (1022, T)):
        p = pyu0.plan(_chain(n, seeds=(1, 2))[0], steps=STEPS, geometry=2)
        assert (p["rc"], p["u0_resident"], p["u0_resident_run"], p["rows"], p["remainder"]) == (0, 1, 1, 1, 0), n
        assert 1 <= p["records"] <= T and (records is None or p["records"] == records), (n, p["records"])
    # one record more than threads (the longest chain the packed geometry holds): the second trip of the streamed loop stays
    p = pyu0.plan(_chain(1023, seeds=(1, 2))[0], steps=STEPS, geometry=2)
    assert (p["rc"], p["top_regs_run"], p["rows"], p["records"], p["u0_resident"], p["u0_resident_run"]) == (0, 1, 1, T + 1, 0, 0)
    # a level 0 that is resident in the slots
    for n in (22, 100):
        p = pyu0.plan(_chain(n)[0], steps=STEPS, geometry=2)
        assert (p["rc"], p["top_regs_run"], p["rows"], p["records"], p["u0_resident"], p["u0_resident_run"]) == (0, 1, 0, 0, 0, 0), n
    # a linear circuit keeps the default program (factor reuse): not the fresh shape at all
    p = pyu0.plan(_chain(1000, kind="rc_ladder")[0], steps=STEPS, geometry=2)
    assert (p["rc"], p["fresh"], p["top_regs"], p["u0_resident"], p["u0_resident_run"]) == (0, 0, 0, 0, 0)
    # ... and where it is given the fresh program, it still reuses its factorisation
    no_knobs.setenv("SPICEY_FRESH_FILL_LINEAR", "1")
    p = pyu0.plan(_chain(1000, kind="rc_ladder")[0], steps=STEPS, geometry=2)
    assert (p["rc"], p["fresh"], p["u0_resident"], p["u0_resident_run"]) == (0, 1, 0, 0)
    no_knobs.delenv("SPICEY_FRESH_FILL_LINEAR")
    # a mesh: level 0 is streamed as generic records
    mesh = abi.flatten(parseNetlist(synth.rcd_mesh(8, 8, tran=".tran 1e-6 7e-5"))).replicate(2)
    p = pyu0.plan(mesh, steps=STEPS, geometry=2)
    assert (p["rc"], p["packed"], p["fresh"], p["rows"], p["u0_resident"], p["u0_resident_run"]) == (0, 1, 1, 0, 0, 0) and p["records"] > 0
    # the other geometries and shapes, and a run beyond the ready-argument kernel's step range
    flat = _chain(1000, seeds=(1, 2))[0]
    lat = pyu0.plan(flat, steps=STEPS, geometry=1)
    assert (lat["rc"], lat["packed"], lat["u0_resident"], lat["u0_resident_run"]) == (0, 0, 0, 0)
    k2 = pyu0.plan(_chain(63, seeds=(1, 2))[0], steps=STEPS, inst_per_wg=2)
    assert (k2["rc"], k2["inst_per_wg"], k2["u0_resident"], k2["u0_resident_run"]) == (0, 2, 0, 0)
    beyond = pyu0.plan(flat, steps=2**32 - 1, geometry=2)
    assert (beyond["u0_resident"], beyond["top_regs_run"], beyond["u0_resident_run"]) == (1, 0, 0)
    # the knob, and the knobs of the forms below it
    for knob in KNOBS[:-1]:
        no_knobs.setenv(knob, "1")
        p = pyu0.plan(flat, steps=STEPS, geometry=2)
        assert p["rc"] == 0 and p["u0_resident_run"] == 0, knob
        if knob in (KNOB, "SPICEY_NO_TOP_REGS"):
            assert p["u0_resident"] == 0, knob
        no_knobs.delenv(knob)
    assert pyu0.plan(flat, steps=STEPS, geometry=2)["u0_resident_run"] == 1


def test_the_decision_on_a_synthetic_descriptor(no_knobs):
    sh = pyu0.shapes()
    take = {"fits": 1, "u0_resident": 1, "u0_resident_run": 1, "shape_u0_resident": 1}
    refuse = {"fits": 0, "u0_resident": 0, "u0_resident_run": 0, "shape_u0_resident": 1}
    for cnt in (1, 2, T - 1, T):
        assert pyu0.decide(1, cnt) == take, cnt
    assert pyu0.decide(1, T + 1) == refuse          # more than T row records
    assert pyu0.decide(1, 0) == refuse              # none
    assert pyu0.decide(1, T, rcnt=1) == refuse      # a generic remainder
    assert pyu0.decide(0, T) == refuse              # generic records
    assert pyu0.decide(1, T, nD=0) == refuse        # a linear circuit (the synthetic header has no switch and no dynamic entry)
    assert pyu0.decide(1, T, top_regs=False) == {**refuse, "fits": 1}
    for name in ("packed_default", "latency"):
        assert sh[name] >= 0 and sh[name] != sh["packed_fresh"]
        d = pyu0.decide(1, T, shape=sh[name], T=512 if name == "packed_default" else 1024)
        assert (d["shape_u0_resident"], d["u0_resident"], d["u0_resident_run"]) == (0, 0, 0), name
    assert pyu0.decide(1, T, shape=-1)["u0_resident"] == 0
    no_knobs.setenv(KNOB, "1")
    assert pyu0.decide(1, T) == {**refuse, "fits": 1}


def test_the_record_words_and_a_second_run(no_knobs):
    """Every thread holds the program's own record `tid` of level 0, a thread at or beyond the record count holds zeros
    (from registers that started as all ones); a second run that starts from the first one's end state, and a run after
    new element values, hold the same record (the topology decides it) and give the bits of the fetching build."""
    flat, dt, src = _chain(766, seeds=(1, 2, 3))   # T - 1 records: thread 511 is the one beyond the count
    first = pyu0.run(flat, STEPS, dt, src, resident=True, nan_fill=True)
    assert first["status"] == 0 and (first["rows"], first["records"], first["remainder"], first["fits"]) == (1, T - 1, 0, 1)
    raw = first["raw"]
    assert raw[: T - 1].any(axis=1).all() and not raw[T - 1:].any()
    assert ((raw[: T - 1, 0] >> 24) & 0x80).all() or (raw[: T - 1, 0] >> 16).all()  # (every record carries flags in its meta half)
    for g in range(flat.n_inst):
        assert np.array_equal(first["u0"][g], raw), g
    assert not first["u0"][:, T - 1:].any()
    off = pyu0.run(flat, STEPS, dt, src, resident=False, nan_fill=True)
    _same(first, off, "first run")
    assert not off["u0"].any()  # (the fetching build clears the words behind every factor phase)
    second = pyu0.run(flat, STEPS, dt, src, resident=True, state=first["state"])
    second_off = pyu0.run(flat, STEPS, dt, src, resident=False, state=off["state"])
    _same(second, second_off, "second run")
    assert np.array_equal(second["u0"], first["u0"]) and not np.array_equal(second["out_v"], first["out_v"])
    flat.R_val[:] = flat.R_val * 1.25
    flat.D_is[:] = flat.D_is * 2.0
    third = pyu0.run(flat, STEPS, dt, src, resident=True)
    third_off = pyu0.run(flat, STEPS, dt, src, resident=False)
    _same(third, third_off, "new element values")
    assert np.array_equal(third["u0"], first["u0"]) and not np.array_equal(third["out_v"], first["out_v"])


def test_a_singular_pivot_below_the_top_reports_the_same_instance(no_knobs):
    """Instance 1 of three has node 501 of a 1000-node chain cut off (tests/test_u0_resident_gpu.py runs the same circuit
    on the GPU): both forms name the same instance, step and iteration."""
    flat, dt, src = _half_clamped_chain(1000)
    node = 501
    flat.R_val[1, (flat.R_n1 == node) | (flat.R_n2 == node)] = 1e16
    flat.C_val[1, (flat.C_n1 == node) | (flat.C_n2 == node)] = 1e-30
    assert pyu0.plan(flat, steps=STEPS, geometry=2)["u0_resident_run"] == 1
    on = pyu0.run(flat, 4, dt, src[:5], resident=True)
    off = pyu0.run(flat, 4, dt, src[:5], resident=False)
    assert on["status"] == abi.ERR_SINGULAR and on["err4"].tolist() == [1, 1, 0, 0]
    assert off["status"] == on["status"] and np.array_equal(on["err4"], off["err4"])
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(on[k][0], off[k][0]), k


def _ulps(a, b):
    ia, ib = a.view(np.int64), b.view(np.int64)
    return np.abs(ia - ib)


def test_the_port_of_exp_as_the_host_compiles_it():
    """spicey_exp_port with the host's fma, rint and ldexp against the host's exp over the diode's argument range
    [-45, 35] (the clamped junction voltage [-1, 0.8] times 1 / (N VT), with margin).  Both are good to less than one
    unit in the last place, so they differ by at most two.  Measured with g++ 13 / glibc: worst difference 1 ulp."""
    rng = np.random.default_rng(19)
    x = np.concatenate([np.linspace(-45.0, 35.0, 1 << 16), rng.uniform(-45.0, 35.0, 1 << 16), rng.uniform(-1e-3, 1e-3, 1 << 10)])
    port, libm = pyu0.exp_pair(x)
    worst = int(_ulps(port, libm).max())
    print(f"exp port against the host's exp on {x.size} arguments in [-45, 35]: worst difference {worst} ulp")
    assert worst <= 2
    # the edges of the port's own range tests
    edge = np.array([0.0, -0.0, np.inf, -np.inf, 709.78, 1024.0, 1025.0, -745.0, -1075.0, -1076.0, np.nextafter(1024.0, np.inf), np.nextafter(-1075.0, -np.inf)])
    port, libm = pyu0.exp_pair(edge)
    assert port[0] == 1.0 and port[1] == 1.0 and port[2] == np.inf and port[3] == 0.0 and port[6] == np.inf and port[9] == 0.0
    assert port[10] == np.inf and port[11] == 0.0
    assert _ulps(port[4:5], libm[4:5]).max() <= 2
    assert np.isnan(pyu0.exp_pair(np.array([np.nan]))[0][0])

