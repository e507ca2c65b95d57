"""Every transient entry point on the packed kernel's fused forms, on the GPU.

The forms of the packed transient kernel (ready arguments, operand addresses, register-exchange top, resident level-0 record,
folded last factor level, stamp fuse) each came with a test of Handle.run with all node voltages recorded and one dt.  One
launch path (spicey_abi.cpp: run_device_src -> enqueue_kernel) serves every other entry point too, and those change what the
forms moved into registers, prologue-built records and host-built tables: a probe filter (the resident `ox` words, ground as
0xFFFF), per-instance diode parameters (the instance index of dpar and zpar), another dt on the same handle (gc = C / dt in
zpar and in the fuse's registers), substituted element values (run_mc, run_sens, run_levels: zpar_fill, statv, rcoef, dpar,
the prologue's stamps of step 0, the fuse's re-deal of statv), a caller's stream, and the shards of a MultiHandle.

Circuits, the knob ladder and the forms each ladder level must report are those of tests/test_packed_forms_entry_points.py,
which checks them on the CPU first.  Every handle here asserts the forms it reports (stamp_fuse_form, top_fold_form,
u0_resident_form, top_regs_form, info()["operand_addr"]), so a plan change cannot turn a test into one of the old kernel.

Two bars.  Byte identity: the program's summation order is fixed and every form states "the parent's bytes", so every ladder
level returns identical bytes in every array an entry point gives back.  The oracle: |x - ref| <= 1e-9 |ref| + 1e-12
(SURVEY.md §8(d)), iteration counts identical; each comparison prints the share of that bar it used ("forms-ratio ...")."""
from __future__ import annotations

import numpy as np
import pytest

from batch_variants import instance
from conftest import bits_equal
from spicey_amd import abi, measure as M, synth
from spicey_amd import tran_mc as tm
from spicey_amd import tran_sens as ts
from spicey_amd.mc import icdf_table
from spicey_amd.measure import fourier, power, rise_time, stats, when
from spicey_amd.netlist import parseNetlist
from test_fourier_gpu import _device_fourier
from test_measure_gpu import _device_measure
from test_packed_forms_entry_points import (BASE_FORMS, FILTERS, HALF, LEVEL_IDS, LEVELS, N, STEPS, TRAN, WHEN_LEVEL, chain, chain_circuit, expected_forms,
                                            ladder, mesh, meets_oracle, second_run_sources, select_columns, set_level, with_state)
from test_power_gpu import _device_power
from test_stamp_fuse import chain_with_bare_node
from test_timing_gpu import _device_timing
from test_tran_mc_gpu import _tol
from tran_mc_host import pytmc as pt
from tran_sens_host import pytsens as ps

pytestmark = pytest.mark.gpu

FULL_LADDER = tuple(range(len(LEVELS)))
STATE_KEYS = ("C_vprev", "L_iprev", "D_vdprev", "S_ison")


@pytest.fixture(scope="module", autouse=True)
def _torch_opens_the_device_first():
    """The device passes and the caller's stream go through torch tensors, the first tests here through handles: in a process
    that runs this file alone torch has to open the device before the library does (spicey_amd/lib.py, load())."""
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()


# ---- handles on the ladder ----------------------------------------------------------------------------------------------------
def _forms(h, steps):
    return (int(h.stamp_fuse_form(steps)), int(h.top_fold_form(steps)), int(h.u0_resident_form(steps)), int(h.top_regs_form(steps)), int(h.info()["operand_addr"]))


def _open(flat, name, level, steps=STEPS):
    """A fresh packed handle under the environment set before the call; the forms it reports are those LEVELS[level] must give."""
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=2)
    try:
        info = h.info()
        assert (info["geometry"], info["threads"], info["resident_slots"], info["inst_per_wg"]) == (2, 512, 4, 1), info
        assert _forms(h, steps) == expected_forms(BASE_FORMS[name], level), (name, LEVEL_IDS[level], _forms(h, steps))
    except BaseException:
        h.close()
        raise
    return h


def _on_ladder(monkeypatch, name, flat, call, levels=FULL_LADDER, steps=STEPS):
    """call(handle) on a fresh handle per ladder level, the knobs set before the handle is created -> the results, in `levels`' order"""
    out = []
    try:
        for level in levels:
            set_level(monkeypatch, level)
            h = _open(flat, name, level, steps)
            try:
                out.append(call(h))
            finally:
                h.close()
    finally:
        set_level(monkeypatch, 0)
    return out


def _on_top(monkeypatch, name, flat, call, steps=STEPS):
    return _on_ladder(monkeypatch, name, flat, call, levels=(0,), steps=steps)[0]


def _same(got, ref, what, keys):
    """Two results of one entry point: status, detail, per-instance status, the arrays `keys`, iteration counts, solve count
    and end state, byte for byte."""
    assert got["status"] == ref["status"] and got["detail"] == ref["detail"], (what, got["detail"], ref["detail"])
    assert np.array_equal(got["inst_status"], ref["inst_status"]), what
    for k in tuple(keys) + ("iters",):
        assert (got[k] is None) == (ref[k] is None), (what, k)
        if ref[k] is not None:
            assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), (what, k, _first_difference(got[k], ref[k]))
    assert ("state" in got) == ("state" in ref), what
    for k, v in ref.get("state", {}).items():
        assert np.asarray(got["state"][k]).tobytes() == np.asarray(v).tobytes(), (what, "state", k)
    if "solves" in ref:
        assert got["solves"] == ref["solves"], what


def _first_difference(a, b):
    """Index (instance, step or row, column) of the first element whose bytes differ, for the assertion's message."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    w = a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,))
    idx = np.argwhere(w.any(axis=-1))
    return tuple(int(i) for i in idx[0]) if len(idx) else None


def _ladder_agrees(results, levels, what, keys):
    for level, r in zip(levels[1:], results[1:]):
        _same(r, results[0], (what, LEVEL_IDS[level]), keys)


# ---- 1. a probe filter ----------------------------------------------------------------------------------------------------------
# name: (circuit, its builder, the recorded nodes, with currents)
PROBE_CASES = {
    "chain_three": ("chain", lambda nodes: chain(3, nodes), FILTERS["three"], True),
    "chain_three_no_currents": ("chain", lambda nodes: chain(3, nodes), FILTERS["three"], False),
    "chain_ground_repeat": ("chain", lambda nodes: chain(3, nodes), FILTERS["ground_repeat"], True),
    "chain_ground_repeat_no_currents": ("chain", lambda nodes: chain(3, nodes), FILTERS["ground_repeat"], False),
    "chain_reverse": ("chain", lambda nodes: chain(3, nodes), FILTERS["reverse"], True),
    "chain_reverse_no_currents": ("chain", lambda nodes: chain(3, nodes), FILTERS["reverse"], False),
    "ladder": ("ladder", ladder, [0, 1000, 3, 1000, 517, 1], True),
    "mesh": ("mesh", mesh, [144, 0, 1, 77, 77], True),
}


@pytest.mark.parametrize("case", sorted(PROBE_CASES))
def test_a_probe_filter(case, oracle_backend, monkeypatch):
    """Ground, a repeated node and reverse order in out_nodes: the ladder's bytes, the column selection of the unfiltered run
    of the same kernel (a +0.0 column for ground; currents, iteration counts and end state untouched by the filter), and every
    instance against the oracle."""
    name, make, nodes, currents = PROBE_CASES[case]
    flat, dt, src = make(nodes)
    everything, _, _ = make(None)
    assert flat.n_out == len(nodes) and everything.n_out == everything.n_nodes and max(nodes) <= flat.n_nodes
    keys = ("out_v", "out_i")
    runs = _on_ladder(monkeypatch, name, flat, lambda h: h.run(STEPS, dt, src, want_currents=currents))
    top = runs[0]
    assert top["status"] == 0 and top["out_v"].shape == (flat.n_inst, STEPS + 1, len(nodes)) and (top["out_i"] is None) == (not currents)
    _ladder_agrees(runs, FULL_LADDER, case, keys)
    full = _on_top(monkeypatch, name, everything, lambda h: h.run(STEPS, dt, src, want_currents=currents))
    assert full["status"] == 0
    want = select_columns(full["out_v"], nodes)
    assert top["out_v"].tobytes() == want.tobytes(), (case, _first_difference(top["out_v"], want))
    if 0 in nodes:
        col = top["out_v"][:, :, nodes.index(0)]
        assert not col.any() and not np.signbit(col).any()
    _same(top, full, (case, "unfiltered"), ("out_i",))
    if name == "ladder":
        assert flat.nS > 0 and int(top["iters"].max()) > 1
    worst = 0.0
    for j in range(flat.n_inst):
        ref = oracle_backend.run(instance(flat, j), STEPS, dt, src, want_currents=currents)
        assert ref["status"] == 0
        worst = max(worst, meets_oracle(top, j, ref, f"probe filter {case}", currents=currents))
    print(f"forms-ratio probe filter {case}: worst {worst:.3g}")


# ---- 2. per-instance diode parameters --------------------------------------------------------------------------------------------
def test_per_instance_diode_parameters(oracle_backend, monkeypatch):
    flat, dt, src = chain(3)
    assert not np.array_equal(flat.D_is[0], flat.D_is[1]) and not np.array_equal(flat.D_is[1], flat.D_is[2]) and not np.array_equal(flat.D_n[1], flat.D_n[2])
    runs = _on_ladder(monkeypatch, "chain", flat, lambda h: h.run(STEPS, dt, src))
    top = runs[0]
    assert top["status"] == 0, top["detail"]
    _ladder_agrees(runs, FULL_LADDER, "diode parameters", ("out_v", "out_i"))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(top["out_v"][a], top["out_v"][b]) and not np.array_equal(top["state"]["D_vdprev"][a], top["state"]["D_vdprev"][b])
    worst = 0.0
    for j in range(3):
        ref = oracle_backend.run(instance(flat, j), STEPS, dt, src)
        assert ref["status"] == 0
        worst = max(worst, meets_oracle(top, j, ref, "diode parameters"))
    # the diode parameters alone tell the instances apart: the R and C of seed 1 in every instance
    same_rc, _, _ = chain(3, replicated=True)
    alone = _on_ladder(monkeypatch, "chain", same_rc, lambda h: h.run(STEPS, dt, src), levels=(0, 7))
    _ladder_agrees(alone, (0, 7), "diode parameters alone", ("out_v", "out_i"))
    assert not np.array_equal(alone[0]["out_v"][0], alone[0]["out_v"][1]) and not np.array_equal(alone[0]["out_v"][1], alone[0]["out_v"][2])
    for j in (1, 2):
        ref = oracle_backend.run(instance(same_rc, j), STEPS, dt, src)
        worst = max(worst, meets_oracle(alone[0], j, ref, "diode parameters alone"))
    print(f"forms-ratio diode parameters: worst {worst:.3g}")


# ---- 3. a second run with another dt ---------------------------------------------------------------------------------------------
def test_a_second_run_with_another_dt(oracle_backend, monkeypatch):
    """HALF steps at dt, then HALF steps at dt / 2 with the sources' values at those times, on one handle per ladder level."""
    from spicey_amd.lib import Handle
    flat, dt, src = chain(3)
    src1 = src[: HALF + 1]
    src2 = second_run_sources(chain_circuit(), HALF * dt, dt / 2, HALF)
    assert np.array_equal(src2[0], src1[HALF])
    keys = ("out_v", "out_i")
    pairs = _on_ladder(monkeypatch, "chain", flat, lambda h: (h.run(HALF, dt, src1), h.run(HALF, dt / 2, src2)), steps=HALF)
    (r1, r2) = pairs[0]
    assert r1["status"] == 0 and r2["status"] == 0, (r1["detail"], r2["detail"])
    for level, (a, b) in zip(FULL_LADDER[1:], pairs[1:]):
        _same(a, r1, ("run 1", LEVEL_IDS[level]), keys)
        _same(b, r2, ("run 2", LEVEL_IDS[level]), keys)
    assert not np.array_equal(r1["out_v"], r2["out_v"])

    def from_the_state(step):
        def call(h):
            h.set_state(r1["state"])
            return h.run(HALF, step, src2)
        return _on_top(monkeypatch, "chain", flat, call, steps=HALF)
    _same(from_the_state(dt / 2), r2, "a fresh handle from run 1's state", keys)
    same_dt = from_the_state(dt)
    assert same_dt["status"] == 0 and not np.array_equal(same_dt["out_v"], r2["out_v"]) and not np.array_equal(same_dt["state"]["C_vprev"], r2["state"]["C_vprev"])
    worst = 0.0
    for j in range(3):
        ref = oracle_backend.run(instance(with_state(flat, r1["state"]), j), HALF, dt / 2, src2)
        assert ref["status"] == 0
        worst = max(worst, meets_oracle(r2, j, ref, "second run at dt / 2"))
    print(f"forms-ratio second run at dt / 2: worst {worst:.3g}")


# ---- 4. run_reduced and the measure family ---------------------------------------------------------------------------------------
MEASURES = {"s": stats(f"v(n{N})"), "m": stats("v(n256)", t_from=3e-5), "tr": rise_time("v(n128)"), "w": when("v(n64)", WHEN_LEVEL), "p": power("R1")}
ROWS = ("meas", "four", "timing", "power")


def _measure_case(n_inst, with_fourier, replicated=False):
    """CHAIN with the recorded nodes of MEASURES -> (flat, dt, src, the resolved plan)"""
    ckt = chain_circuit()
    flat, dt, src = chain(n_inst, replicated=replicated)
    measures = dict(MEASURES, f=fourier("v(n64)", f0=1.0 / (32 * dt), harmonics=3)) if with_fourier else MEASURES
    plan = M._Plan(ckt, measures, dt, STEPS)
    assert plan.need_i and plan.out_nodes == [1, 2, 64, 128, 256, N] and (len(plan.reqs), len(plan.treqs), len(plan.preqs), len(plan.freqs)) == (2, 2, 1, int(with_fourier))
    flat.out_nodes = np.ascontiguousarray(plan.out_nodes, dtype=np.int32)
    return flat, dt, src, plan


def test_the_when_threshold_is_crossed_inside_the_run(oracle_backend):
    flat, dt, src, plan = _measure_case(4, False)
    col = plan.out_nodes.index(64)
    for j in range(4):
        v = oracle_backend.run(instance(flat, j), STEPS, dt, src)["out_v"][0][:, col]
        up = np.nonzero((v[:-1] < WHEN_LEVEL) & (v[1:] >= WHEN_LEVEL))[0]
        assert len(up) == 1 and 8 <= up[0] <= STEPS - 9, (j, up)


def test_run_reduced_and_the_measure_family(monkeypatch):
    """The rows of every pass, iteration counts and end state over the ladder; the top level's rows against the standalone device
    passes over that level's own waveforms (held to the oracle in test_a_probe_filter), and against the positional entry points."""
    flat, dt, src, plan = _measure_case(4, True)
    reduced = _on_ladder(monkeypatch, "chain", flat, lambda h: h.run_reduced(STEPS, dt, src, plan.reqs, plan.freqs, plan.treqs, (), plan.preqs))
    top = reduced[0]
    assert top["status"] == 0 and (top["inst_status"] == 0).all(), top["detail"]
    _ladder_agrees(reduced, FULL_LADDER, "run_reduced", ROWS)
    for a, b in ((0, 1), (1, 2), (2, 3)):
        assert not np.array_equal(top["meas"][a], top["meas"][b])
    wave = _on_top(monkeypatch, "chain", flat, lambda h: h.run(STEPS, dt, src))
    assert wave["status"] == 0 and np.array_equal(wave["iters"], top["iters"])
    for k in STATE_KEYS:
        assert np.asarray(wave["state"][k]).tobytes() == np.asarray(top["state"][k]).tobytes(), k
    v, i = wave["out_v"], wave["out_i"]
    alone = {"meas": _device_measure(v, i, plan.reqs, dt), "four": _device_fourier(v, i, plan.freqs, dt), "timing": _device_timing(v, i, plan.treqs, dt),
             "power": _device_power(v, i, plan.preqs, dt)}
    for k in ROWS:
        assert top[k].shape == alone[k].shape and bits_equal(top[k], alone[k]).all(), (k, _first_difference(top[k], alone[k]))
    # the threshold was found where the waveform crosses it: one crossing per instance, inside the run
    w = top["timing"][:, 1]
    assert (w[:, 7] == 1).all() and (w[:, 4] > 8 * dt).all() and (w[:, 4] < (STEPS - 8) * dt).all(), w
    # the positional entry points of the family give the rows of the struct's

    def family(h):
        out = [h.run_measure(STEPS, dt, src, plan.reqs)]
        for call in (lambda: h.run_measure_fourier(STEPS, dt, src, plan.reqs, plan.freqs), lambda: h.run_measure_timing(STEPS, dt, src, plan.reqs, plan.freqs, plan.treqs),
                     lambda: h.run_measure_power(STEPS, dt, src, plan.reqs, plan.freqs, plan.treqs, [], plan.preqs)):
            h.reset_state()
            out.append(call())
        return out
    for level, results in zip((0, 7), _on_ladder(monkeypatch, "chain", flat, family, levels=(0, 7))):
        for r, rows in zip(results, (ROWS[:1], ROWS[:2], ROWS[:3], ROWS)):
            _same(r, top, ("measure family", LEVEL_IDS[level], rows), rows)


# ---- 5. run_mc -----------------------------------------------------------------------------------------------------------------
def _rows_of(r, plan):
    return (r["meas"] if len(plan.reqs) else None, r["timing"] if len(plan.treqs) else None, r["power"] if len(plan.preqs) else None)


def _reduced_under_all_knobs(monkeypatch, values, dt, src, plan):
    """run_reduced of a handle created from `values` with every knob set: the oldest packed kernel, which reads them where they lie"""
    r = _on_ladder(monkeypatch, "chain", values, lambda h: h.run_reduced(STEPS, dt, src, plan.reqs, (), plan.treqs, (), plan.preqs), levels=(7,))[0]
    r["rows"] = _rows_of(r, plan)
    return r


def test_run_mc(oracle_backend, monkeypatch):
    """Drawn R and C in the place of the handle's own, on the kernel that keeps what it derives from them in registers and
    records: the ladder's bytes; a second handle created from the numpy draw's values with every knob set; the nominal sample;
    an open quantile band; the handle's own values back afterwards; two drawn samples against the oracle."""
    flat, dt, src, plan = _measure_case(5, False, replicated=True)
    names, sc, root = tm.compile_plan(plan, dt)
    icdf, log2K = icdf_table("gauss")
    req = abi.tran_mc_req(log2K, True, 2025)
    tol = _tol(flat)
    lo, hi = np.full(len(names), -np.inf), np.full(len(names), np.inf)
    hi[0] = 1e300
    lists = (plan.reqs, (), plan.treqs, (), plan.preqs)

    def call(h):
        before = h.run_reduced(STEPS, dt, src, *lists)
        h.reset_state()
        res = h.run_mc(STEPS, dt, src, req, tol, icdf, sc, lo, hi, pt.PROBS, plan.reqs, plan.treqs, plan.preqs, want_x=True, want_iters=True)
        h.reset_state()
        after = h.run_reduced(STEPS, dt, src, *lists)
        return before, res, after
    runs = _on_ladder(monkeypatch, "chain", flat, call)
    before, top, after = runs[0]
    assert before["status"] == abi.OK and top["status"] == abi.OK and (top["inst_status"] == 0).all(), top["detail"]
    for level, (b, r, a) in zip(FULL_LADDER, runs):
        _same(r, top, ("run_mc", LEVEL_IDS[level]), ("x", "stat", "sample"))
        _same(b, before, ("run_reduced before run_mc", LEVEL_IDS[level]), ROWS)
        _same(a, before, ("run_reduced after run_mc", LEVEL_IDS[level]), ROWS)  # the handle's own values and records are back
    ref = pt.run_mc_reference(lambda drawn: _reduced_under_all_knobs(monkeypatch, drawn, dt, src, plan), flat, STEPS, dt, src, req, tol, icdf, sc, lo, hi, pt.PROBS, reducer="numpy")
    assert ref["status"] == abi.OK and (ref["inst_status"] == 0).all()
    assert pt.bits_equal(top["x"], ref["x"]).all(), _first_difference(top["x"], ref["x"])
    assert (top["sample"] == ref["sample"]).all() and pt.bits_equal(top["stat"], ref["stat"]).all()
    assert np.array_equal(top["iters"], ref["run"]["iters"])
    for k in STATE_KEYS:  # the end state is the drawn run's
        assert np.asarray(top["state"][k]).tobytes() == np.asarray(ref["state"][k]).tobytes(), k
    # sample 0 is the nominal circuit; the draw did reach the kernel: some scalar's quantile band is open, and the drawn run differs
    assert pt.bits_equal(top["x"][0], tm.eval_reference_scalars(sc, _rows_of(before, plan))[0]).all()
    assert bool((top["stat"][:, 8] < top["stat"][:, 8 + 2 * len(pt.PROBS) - 1]).any())
    assert not np.array_equal(top["state"]["C_vprev"][1], before["state"]["C_vprev"][1])
    # independently: the top-level kernel on handles created from the drawn values, against the oracle of those values
    drawn = pt.drawn_flat(flat, tol, icdf, req)
    assert not np.array_equal(drawn.R_val[1], flat.R_val[1]) and np.array_equal(drawn.R_val[0], flat.R_val[0])
    plain = _on_top(monkeypatch, "chain", drawn, lambda h: h.run(STEPS, dt, src))
    assert plain["status"] == 0
    for k in STATE_KEYS:
        assert np.asarray(plain["state"][k]).tobytes() == np.asarray(top["state"][k]).tobytes(), k
    worst = 0.0
    for j in (1, 4):
        ref_j = oracle_backend.run(instance(drawn, j), STEPS, dt, src)
        assert ref_j["status"] == 0
        worst = max(worst, meets_oracle(plain, j, ref_j, "drawn sample"))
    print(f"forms-ratio run_mc drawn samples: worst {worst:.3g}")


# ---- 6. run_sens and run_levels ----------------------------------------------------------------------------------------------------
def test_run_sens_and_run_levels(oracle_backend, monkeypatch):
    """One-at-a-time steps of eight elements spread along the chain (R1, R255, R256, R510 — the chain's last resistor; it has no
    R511 —, C1, C128, C256, C510) and a levels design with a mixed +-1 pattern: the ladder's bytes, and a second handle created
    from the numpy design's values with every knob set, its rows through the numpy scalars and reduction.  The instances of the
    sensitivity run share the nominal diode parameters (a sensitivity compares like with like); those of the levels run, which
    reduces nothing, keep CHAIN's per-instance ones."""
    flat5, dt, src, plan = _measure_case(5, False, replicated=True)
    names, sc, root = tm.compile_plan(plan, dt)
    nR = flat5.nR
    act = np.array([0, 254, 255, 509, nR + 0, nR + 127, nR + 255, nR + 509], np.int32)
    nA = len(act)
    tol = np.zeros(flat5.nR + flat5.nC + flat5.nL)
    tol[act] = np.where(act < nR, 0.02, 0.05)
    step = np.where(np.arange(nA) % 2 == 0, 1e-3, 2e-3)
    flat = instance(flat5, 0).replicate(1 + 2 * nA)
    assert flat.n_inst == 17 and np.array_equal(flat.out_nodes, flat5.out_nodes)
    req = abi.tran_sens_req(abi.TS_ONE_AT_A_TIME, nA)
    lists = (plan.reqs, (), plan.treqs, (), plan.preqs)
    levels = FULL_LADDER

    def call(h):
        before = h.run_reduced(STEPS, dt, src, *lists)
        h.reset_state()
        res = h.run_sens(STEPS, dt, src, req, act, step, tol, sc, plan.reqs, plan.treqs, plan.preqs, want_x=True, want_iters=True)
        h.reset_state()
        after = h.run_reduced(STEPS, dt, src, *lists)
        return before, res, after
    runs = _on_ladder(monkeypatch, "chain", flat, call, levels=levels)
    before, top, after = runs[0]
    assert before["status"] == abi.OK and top["status"] == abi.OK and (top["inst_status"] == 0).all(), top["detail"]
    for level, (b, r, a) in zip(levels, runs):
        _same(r, top, ("run_sens", LEVEL_IDS[level]), ("x", "sens", "sign", "bound"))
        _same(b, before, ("run_reduced before run_sens", LEVEL_IDS[level]), ROWS)
        _same(a, before, ("run_reduced after run_sens", LEVEL_IDS[level]), ROWS)
    designed = ps.designed_flat(flat, act, step)
    assert not np.array_equal(designed.R_val[1], flat.R_val[1]) and np.array_equal(designed.R_val[0], flat.R_val[0])
    ref = _reduced_under_all_knobs(monkeypatch, designed, dt, src, plan)
    assert ref["status"] == abi.OK
    rx = tm.eval_reference_scalars(sc, ref["rows"])
    rsens, rsign, rbound = ts.reduce_reference_tran_sens(rx, None, step, tol[act])
    assert ps.bits_equal(top["x"], rx).all(), _first_difference(top["x"], rx)
    assert ps.bits_equal(top["sens"], rsens).all() and (top["sign"] == rsign).all() and ps.bits_equal(top["bound"], rbound).all()
    assert np.array_equal(top["iters"], ref["iters"])
    for k in STATE_KEYS:
        assert np.asarray(top["state"][k]).tobytes() == np.asarray(ref["state"][k]).tobytes(), k
    assert pt.bits_equal(top["x"][0], tm.eval_reference_scalars(sc, _rows_of(before, plan))[0]).all()
    # the designed values did reach the run: every element moves some scalar, and the element next to the source moves v(n64)'s crossing
    assert (top["sign"] != 0).any(axis=0).all()
    assert top["x"][1, names.index("w.t")] != top["x"][2, names.index("w.t")]
    # a perturbed instance on the top-level kernel against the oracle of its values: C510 up, the far end of the chain
    j = 1 + 2 * (nA - 1)
    plain = _on_top(monkeypatch, "chain", designed, lambda h: h.run(STEPS, dt, src))
    ref_j = oracle_backend.run(instance(designed, j), STEPS, dt, src)
    assert plain["status"] == 0 and ref_j["status"] == 0
    worst = meets_oracle(plain, j, ref_j, "designed instance")
    # the levels design, on CHAIN's five instances with their own diode parameters
    lreq = abi.tran_sens_req(abi.TS_LEVELS, 0)
    ltol = np.concatenate([np.full(flat5.nR, 0.02), np.full(flat5.nC, 0.05)])
    pattern = np.where((np.arange(len(ltol)) // 3) % 2 == 0, 1, -1).astype(np.int8)
    lvl = np.stack([np.zeros_like(pattern), pattern, -pattern, np.roll(pattern, 1), np.where(np.arange(len(ltol)) % 5 == 0, 0, pattern).astype(np.int8)])
    assert lvl.shape == (5, len(ltol)) and (lvl[1:] == 1).any(axis=1).all() and (lvl[1:] == -1).any(axis=1).all()
    lruns = _on_ladder(monkeypatch, "chain", flat5, lambda h: h.run_levels(STEPS, dt, src, lreq, lvl, ltol, sc, plan.reqs, plan.treqs, plan.preqs, want_iters=True), levels=levels)
    ltop = lruns[0]
    assert ltop["status"] == abi.OK and (ltop["inst_status"] == 0).all(), ltop["detail"]
    _ladder_agrees(lruns, levels, "run_levels", ("x",))
    ldesigned = ps.designed_flat(flat5, lvl=lvl, tol=ltol)
    lref = _reduced_under_all_knobs(monkeypatch, ldesigned, dt, src, plan)
    assert lref["status"] == abi.OK and ps.bits_equal(ltop["x"], tm.eval_reference_scalars(sc, lref["rows"])).all()
    for k in STATE_KEYS:
        assert np.asarray(ltop["state"][k]).tobytes() == np.asarray(lref["state"][k]).tobytes(), k
    nominal = _on_top(monkeypatch, "chain", flat5, lambda h: h.run_reduced(STEPS, dt, src, *lists))
    assert ps.bits_equal(ltop["x"][0], tm.eval_reference_scalars(sc, _rows_of(nominal, plan))[0]).all()
    assert not ps.bits_equal(ltop["x"][1:], tm.eval_reference_scalars(sc, _rows_of(nominal, plan))[1:]).all(axis=1).any()
    lplain = _on_top(monkeypatch, "chain", ldesigned, lambda h: h.run(STEPS, dt, src))
    ref_3 = oracle_backend.run(instance(ldesigned, 3), STEPS, dt, src)
    assert lplain["status"] == 0 and ref_3["status"] == 0
    worst = max(worst, meets_oracle(lplain, 3, ref_3, "levels instance"))
    print(f"forms-ratio run_sens and run_levels: worst {worst:.3g}")


# ---- 7. a caller's stream, and shards ----------------------------------------------------------------------------------------------
def _own_sources(src, n_inst):
    per = np.ascontiguousarray(np.stack([src * s for s in (1.0, 0.6, -0.4, 0.8)[:n_inst]]))  # (a bipolar one among them: its diodes stay off)
    assert per.shape == (n_inst,) + src.shape
    return per


def test_run_device_on_a_callers_stream(monkeypatch):
    """spicey_run_device_src on a torch stream that is not the default one, source tables per instance on the device: the bytes
    of Handle.run with the same tables."""
    import torch
    flat, dt, src = chain(4)
    per = _own_sources(src, 4)
    host = _on_top(monkeypatch, "chain", flat, lambda h: h.run(STEPS, dt, per))
    assert host["status"] == 0 and not np.array_equal(host["out_v"][0], host["out_v"][1])

    def call(h):
        stream = torch.cuda.Stream()
        assert stream.cuda_stream != 0 and stream != torch.cuda.default_stream()
        d_src = torch.from_numpy(per).cuda()
        d_v = torch.full((4, STEPS + 1, flat.n_out), float("nan"), dtype=torch.float64, device="cuda")
        d_i = torch.full((4, STEPS + 1, flat.n_cur), float("nan"), dtype=torch.float64, device="cuda")
        d_it = torch.full((4, STEPS + 1), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        try:
            h.run_device(STEPS, dt, d_src.data_ptr(), d_v.data_ptr(), d_i.data_ptr(), d_it.data_ptr(), stream=stream.cuda_stream, src_per_inst=True)
            assert h.sync() == 0, h.error()
        finally:
            stream.synchronize()
            torch.cuda.synchronize()
        return {"status": 0, "detail": "", "inst_status": h.inst_status(), "out_v": d_v.cpu().numpy(), "out_i": d_i.cpu().numpy(), "iters": d_it.cpu().numpy(),
                "state": h.state(), "solves": h.solves()}
    for level, got in zip((0, 7), _on_ladder(monkeypatch, "chain", flat, call, levels=(0, 7))):
        _same(got, host, ("run_device on a stream", LEVEL_IDS[level]), ("out_v", "out_i"))


def test_the_shards_of_a_multi_handle(monkeypatch):
    """Two shards of two instances on one device, each a handle of its own: the single handle's bytes, shared and per-instance
    source tables.  SpiceyInfo of a shard says the kernel family (operand addresses, the top's rows); that a two-instance
    plan of this chain fuses is asserted on a Handle of two instances, under the same environment."""
    from spicey_amd.lib import MultiHandle
    flat, dt, src = chain(4)
    per = _own_sources(src, 4)
    single = _on_top(monkeypatch, "chain", flat, lambda h: (h.run(STEPS, dt, src), h.run(STEPS, dt, per)))
    set_level(monkeypatch, 0)
    two = chain(2)[0]
    _open(two, "chain", 0).close()
    m = MultiHandle(flat, [0, 0], geometry=2)
    try:
        shards = m.shards()
        assert [(s["first_inst"], s["n_inst"]) for s in shards] == [(0, 2), (2, 2)]
        for s in shards:
            i = s["info"]
            assert (i["geometry"], i["threads"], i["resident_slots"], i["inst_per_wg"], i["operand_addr"]) == (2, 512, 4, 1, 1), i
        runs = (m.run(STEPS, dt, src), m.run(STEPS, dt, per))
    finally:
        m.close()
    for got, ref, what in zip(runs, single, ("shared sources", "per-instance sources")):
        assert got["status"] == 0 and ref["status"] == 0, got["detail"]
        for k in ("out_v", "out_i", "iters"):
            assert got[k].tobytes() == ref[k].tobytes(), (what, k, _first_difference(got[k], ref[k]))
        for k in STATE_KEYS:
            assert np.asarray(got["state"][k]).tobytes() == np.asarray(ref["state"][k]).tobytes(), (what, k)
        assert got["solves"] == ref["solves"], what
    assert not np.array_equal(runs[0]["out_v"], runs[1]["out_v"])


# ---- 8. a failing sample under substituted values ----------------------------------------------------------------------------------
def test_run_mc_with_a_singular_sample(monkeypatch):
    """The chain with a bare node at n = 511 (it still fuses: tests/test_packed_forms_entry_points.py asserts the plan, and the
    handle its form): sample 1 of three has a pivot of 2e-16 in the matrix of step 0, which the fused form stamps in its
    prologue from the substituted values.  Zero tolerances: the drawn values are the nominal ones.  An error return, the
    condition tests/test_stamp_fuse_gpu.py::test_a_singular_pivot_in_the_stamps_of_step_0 runs: the top level and the oldest
    kernel name the same sample, step and iteration, and leave it out of the statistics."""
    flat, dt, src = chain_with_bare_node(n=N, steps=STEPS)
    lines = [s for s in synth.diode_chain(N, seed=3, tran=TRAN).split("\n") if not s.startswith(("D2 ", "C2 "))]
    ckt = parseNetlist("\n".join(lines))
    assert abi.flatten(ckt).nD == flat.nD == N - 2
    plan = M._Plan(ckt, {"s": stats(f"v(n{N})"), "m": stats("v(n64)")}, dt, STEPS)
    flat.out_nodes = np.ascontiguousarray(plan.out_nodes, dtype=np.int32)
    names, sc, root = tm.compile_plan(plan, dt)
    per = np.ascontiguousarray(np.broadcast_to(src, (3, STEPS + 1, flat.nV)))
    tol = np.zeros(flat.nR + flat.nC + flat.nL)
    req = abi.tran_mc_req(0, True, 1)
    uni = np.array([-1.0, 1.0])

    def call(h):
        res = h.run_mc(STEPS, dt, per, req, tol, uni, sc, None, None, pt.PROBS, plan.reqs, want_x=True, want_iters=True)
        h.reset_state()  # (the samples that finished moved on)
        return res, h.run_reduced(STEPS, dt, per, plan.reqs)
    runs = _on_ladder(monkeypatch, "chain", flat, call, levels=(0, 7))
    (top, plain), (old, old_plain) = runs
    for res in (top, old):
        assert res["status"] == abi.ERR_SINGULAR and "singular at inst 1 step 0" in res["detail"]
        assert np.array_equal(res["inst_status"], [0, abi.ERR_SINGULAR, 0])
        assert (res["stat"][:, 0] == 2).all() and (res["sample"][1] == -1).all() and (np.delete(res["sample"], 1, axis=0) == [0, -1]).all()
        assert np.isnan(res["x"][1]).all() and np.isfinite(res["x"][[0, 2]]).all()
    assert top["detail"] == old["detail"]
    assert pt.bits_equal(top["x"], old["x"]).all() and pt.bits_equal(top["stat"], old["stat"]).all() and (top["sample"] == old["sample"]).all()
    for j in (0, 2):
        assert np.array_equal(top["iters"][j], old["iters"][j]) and top["iters"][j].all()
    # zero tolerances: the scalars are those of the handle's own values
    assert plain["status"] == abi.ERR_SINGULAR and np.array_equal(plain["inst_status"], top["inst_status"]) and plain["detail"] == old_plain["detail"]
    valid = (top["inst_status"] == 0).astype(np.uint8)
    x = tm.eval_reference_scalars(sc, (plain["meas"], None, None), valid)
    sample, stat = tm.reduce_reference_tran_mc(x, valid, None, None, pt.PROBS)
    assert pt.bits_equal(top["x"], x).all() and pt.bits_equal(top["stat"], stat).all() and (top["sample"] == sample).all()
