"""The stamp fuse (tran_v2_run.h: SF — the folded packed kernel whose Z stamps the next step's matrix and right-hand side
from registers, with no phase B in the time loop) on the GPU.

Every case runs on the packed layout (512 threads, 4 slots), 64 steps, with SPICEY_NO_STAMP_FUSE and without, on fresh
handles, and must give the same bytes — voltages, currents, iteration counts, statuses, solve count, end state; the run
without the knob is held against the emulator of this build (tests/stamp_fuse_host: the host form of the fused phases on
the sequential executor) at the project's bar, 1e-9 |ref| + 1e-12.  That emulator runs the host form of the very code under
test: the independent check is the byte comparison with the knob.  Every case says which form it expects
(spicey_stamp_fuse_form of the handle, and the plan's own decision on the CPU): diode_chain(511) is the smallest chain that
takes the fuse, diode_chain(766) has free slots in the second item of half the threads, diode_chain(1000) is the bench
circuit (found on the CPU, tests/test_stamp_fuse.py)."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import abi, synth
from test_gpu_parity import tol_ratio
from test_packed_resident_gpu import _switched_ladder
from test_stamp_fuse import chain_with_bare_node, chain_with_floating_diode, chain_with_inductor, _from_text
from test_top_regs_gpu import _half_clamped_chain
from stamp_fuse_host import pysf

pytestmark = pytest.mark.gpu

STEPS = 64
T = 512
KNOB = "SPICEY_NO_STAMP_FUSE"
OTHER_KNOBS = ("SPICEY_NO_TOP_FOLD", "SPICEY_NO_U0_RESIDENT", "SPICEY_NO_TOP_REGS", "SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS",
               "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL", "SPICEY_FRESH_FILL_LINEAR")
TRAN = f".tran 1e-6 {(STEPS + 6) * 1e-6:.6g}"


def _chain(n, seeds=(1, 2), kind="diode_chain"):
    flat, dt, total, src = synth.chain_batch(kind, n, list(seeds), tran=TRAN)
    assert total >= STEPS
    return flat, dt, src[: STEPS + 1]


def _run(flat, dt, src, runs=1, steps=STEPS, currents=True, **options):
    """-> (results of `runs` consecutive runs of `steps` steps, info(), spicey_stamp_fuse_form for such a run) of a fresh handle"""
    from spicey_amd.lib import Handle
    h = Handle(flat, **options)
    try:
        form = h.stamp_fuse_form(steps)
        r = [h.run(steps, dt, src[: steps + 1] if src.ndim < 3 else src[:, : steps + 1], want_currents=currents) for _ in range(runs)]
        return r, h.info(), form
    finally:
        h.close()


def _both(monkeypatch, flat, dt, src, want, runs=1, steps=STEPS, currents=True, **options):
    """Knob set (phase B stamps), knob not set (Z stamps where the plan says so): what each handle reports, and the same
    plan otherwise."""
    options.setdefault("geometry", 2)
    for k in OTHER_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(KNOB, "1")
    off, info_off, form_off = _run(flat, dt, src, runs, steps, currents, **options)
    p_off = pysf.plan(flat, steps=steps, **options)
    monkeypatch.delenv(KNOB)
    on, info_on, form_on = _run(flat, dt, src, runs, steps, currents, **options)
    p_on = pysf.plan(flat, steps=steps, **options)
    assert info_on == info_off  # the same plan, the same LDS: the knob picks between two kernels of one shape
    assert form_off is False and p_off["rc"] == 0 and (p_off["stamp_fuse"], p_off["stamp_fuse_run"]) == (0, 0)
    assert form_on is bool(want) and p_on["rc"] == 0 and (p_on["stamp_fuse"], p_on["stamp_fuse_run"]) == (int(want), int(want)), (form_on, p_on)
    return off, on, p_on


def _same(off, on, what):
    assert on["status"] == off["status"] and on["detail"] == off["detail"], what
    assert np.array_equal(on["inst_status"], off["inst_status"]), what
    for k in ("out_v", "out_i"):
        assert (on[k] is None) == (off[k] is None), (what, k)
        if on[k] is not None:
            assert on[k].tobytes() == off[k].tobytes(), (what, k)
    assert np.array_equal(on["iters"], off["iters"]), (what, "iters")
    if on["status"] == 0:
        assert on["solves"] == off["solves"], what
        for k, v in off["state"].items():
            assert np.asarray(v).tobytes() == np.asarray(on["state"][k]).tobytes(), (what, "state", k)


def _meets_emulator(got, flat, dt, src, what, steps=STEPS, currents=True):
    ref = pysf.run(flat, steps, dt, src, fuse=True, currents=currents)
    assert ref["status"] == 0 and ref["table_ok"] == 1
    rv = float(tol_ratio(got["out_v"], ref["out_v"]).max())
    ri = float(tol_ratio(got["out_i"], ref["out_i"]).max()) if currents else 0.0
    print(f"stamp-fuse ratio {what}: out_v {rv:.3g} out_i {ri:.3g} of the bar")
    assert rv <= 1.0 and ri <= 1.0, (what, rv, ri)
    assert np.array_equal(got["iters"], ref["iters"]), what


@pytest.mark.parametrize("n", [511, 766, 1000])
def test_a_chain_gives_the_bytes_of_the_kernel_with_phase_b(n, monkeypatch):
    flat, dt, src = _chain(n)
    off, on, plan = _both(monkeypatch, flat, dt, src, True)
    assert (plan["packed"], plan["threads"], plan["top_fold_run"]) == (1, T, 1)
    assert on[0]["status"] == 0, on[0]["detail"]
    assert np.isfinite(on[0]["out_v"]).all() and np.isfinite(on[0]["out_i"]).all() and float(np.abs(on[0]["out_v"]).max()) > 1.0
    _same(off[0], on[0], n)
    _meets_emulator(on[0], flat, dt, src, f"diode_chain({n})")


def test_a_second_run_on_the_handle(monkeypatch):
    """Two runs on one handle: the second starts from the first one's end state, and its prologue stamps from it."""
    flat, dt, src = _chain(1000)
    off, on, plan = _both(monkeypatch, flat, dt, src, True, runs=2)
    assert on[0]["status"] == 0 and on[1]["status"] == 0
    _same(off[0], on[0], "first run")
    _same(off[1], on[1], "second run")
    assert not np.array_equal(on[0]["out_v"], on[1]["out_v"])


def test_three_instances_with_their_own_sources_and_parameters(monkeypatch):
    flat, dt, src = _chain(1000, seeds=(3, 4, 5))
    per = np.ascontiguousarray(np.stack([src * s for s in (1.0, 0.6, -0.4)]))  # (a bipolar one among them: the diodes stay off)
    assert per.shape == (3, STEPS + 1, flat.nV) and not np.array_equal(flat.R_val[0], flat.R_val[1])
    off, on, plan = _both(monkeypatch, flat, dt, per, True)
    assert on[0]["status"] == 0
    _same(off[0], on[0], "three instances")
    assert not np.array_equal(on[0]["out_v"][0], on[0]["out_v"][1]) and not np.array_equal(on[0]["out_v"][1], on[0]["out_v"][2])
    _meets_emulator(on[0], flat, dt, per, "three instances, per-instance sources")


def test_a_run_without_currents(monkeypatch):
    flat, dt, src = _chain(1000)
    off, on, plan = _both(monkeypatch, flat, dt, src, True, currents=False)
    assert on[0]["status"] == 0 and on[0]["out_i"] is None
    _same(off[0], on[0], "no currents")
    _meets_emulator(on[0], flat, dt, src, "no currents", currents=False)


def test_a_run_of_one_step(monkeypatch):
    flat, dt, src = _chain(1000)
    off, on, plan = _both(monkeypatch, flat, dt, src, True, steps=1)
    assert on[0]["status"] == 0 and on[0]["out_v"].shape[1] == 2
    _same(off[0], on[0], "one step")
    _meets_emulator(on[0], flat, dt, src[:2], "one step", steps=1)


def test_a_singular_pivot_is_reported_the_same_way(monkeypatch):
    """The singular instance of the fold's test: instance 1 of three has node 501 of the half-clamped 1000-node chain cut off —
    a pivot of ~2e-16, an error return, not a fault.  That chain has a diode at every other node only, so diode and
    capacitor of one node have different indices and the plan refuses the fuse: both handles run today's form, and must name
    the same instance, step and iteration."""
    flat, dt, src = _half_clamped_chain(1000)
    node = 501
    assert node not in set(flat.D_np) | set(flat.D_nm) | set(flat.V_n1) | set(flat.V_n2)
    flat.R_val[1, (flat.R_n1 == node) | (flat.R_n2 == node)] = 1e16
    flat.C_val[1, (flat.C_n1 == node) | (flat.C_n2 == node)] = 1e-30
    per = np.ascontiguousarray(np.broadcast_to(src, (3, STEPS + 1, flat.nV)))  # (per-instance layout: partial results stand)
    off, on, plan = _both(monkeypatch, flat, dt, per, False)
    on, off = on[0], off[0]
    assert on["status"] == abi.ERR_SINGULAR and "singular at inst 1 step 0" in on["detail"]
    assert np.array_equal(on["inst_status"], [0, abi.ERR_SINGULAR, 0])
    assert on["detail"] == off["detail"] and np.array_equal(on["inst_status"], off["inst_status"])
    for j in (0, 2):
        for k in ("out_v", "out_i", "iters"):
            assert on[k][j].tobytes() == off[k][j].tobytes(), (j, k)
        assert np.isfinite(on["out_v"][j]).all()


def test_a_singular_pivot_in_the_stamps_of_step_0(monkeypatch):
    """A chain that takes the fuse, with a pivot below the bar in the matrix of step 0 (instance 1 of three: node 3 holds two
    resistors of 1e16 ohm and nothing else).  The fused form stamps step 0 in its prologue; it must name the instance, step
    and iteration that phase B's form names, and the instances beside it must finish with the same bytes."""
    flat, dt, src = chain_with_bare_node(steps=STEPS)
    per = np.ascontiguousarray(np.broadcast_to(src, (3, STEPS + 1, flat.nV)))
    off, on, plan = _both(monkeypatch, flat, dt, per, True)
    on, off = on[0], off[0]
    assert on["status"] == abi.ERR_SINGULAR and "singular at inst 1 step 0" in on["detail"]
    assert np.array_equal(on["inst_status"], [0, abi.ERR_SINGULAR, 0])
    assert on["detail"] == off["detail"] and np.array_equal(on["inst_status"], off["inst_status"])
    for j in (0, 2):
        for k in ("out_v", "out_i", "iters"):
            assert on[k][j].tobytes() == off[k][j].tobytes(), (j, k)
        assert np.isfinite(on["out_v"][j]).all()


def test_the_form_is_not_taken_where_its_conditions_fail(monkeypatch):
    for k in OTHER_KNOBS + (KNOB,):
        monkeypatch.delenv(k, raising=False)
    flat, dt, src = _chain(1000)
    on, _, form = _run(flat, dt, src, geometry=2)
    assert form is True and on[0]["status"] == 0
    # a plan without the fold: that form's parent runs, this one does not
    monkeypatch.setenv("SPICEY_NO_TOP_FOLD", "1")
    tr, info, form = _run(flat, dt, src, geometry=2)
    assert form is False and tr[0]["status"] == 0
    monkeypatch.delenv("SPICEY_NO_TOP_FOLD")
    assert tr[0]["out_v"].tobytes() == on[0]["out_v"].tobytes() and tr[0]["out_i"].tobytes() == on[0]["out_i"].tobytes() and np.array_equal(tr[0]["iters"], on[0]["iters"])
    refused = {
        "rc_ladder": _chain(1000, kind="rc_ladder"),
        "switched_ladder": (lambda f, d, s: (f, d, s[: STEPS + 1]))(*_switched_ladder()),
        "inductor": chain_with_inductor(steps=STEPS),
        "rcd_mesh": (lambda f, d, s: (f.replicate(2), d, s))(*_from_text(synth.rcd_mesh(12, tran=TRAN), STEPS)),
        "floating_diode": chain_with_floating_diode(steps=STEPS),
    }
    for what, (f, d, s) in refused.items():
        assert len(s) == STEPS + 1
        assert pysf.plan(f, steps=STEPS, geometry=2)["stamp_fuse_run"] == 0, what
        r, info, form = _run(f, d, s, geometry=2)
        assert form is False and r[0]["status"] == 0, (what, r[0]["detail"])
    # a run beyond the ready-argument kernel's step range has no such form (asked of the handle, not run)
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=2)
    try:
        assert h.stamp_fuse_form(STEPS) is True and h.stamp_fuse_form(2**32 - 1) is False
    finally:
        h.close()
