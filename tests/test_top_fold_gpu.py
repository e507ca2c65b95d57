"""The fold of the last factor level into the tridiagonal top (tran_v2_run.h: TF — the packed resident-record kernel whose
top lanes run the row records of the level below the top themselves and keep a_ii, y_i and the two fills in registers) on
the GPU.

Every case runs on the packed layout (512 threads, 4 slots), 64 steps, all voltages and currents, with SPICEY_NO_TOP_FOLD
and without, on fresh handles, and must give the same bytes — voltages, currents, iteration counts, statuses, solve count,
end state; the run without the knob is held against the emulator of this very build (tests/top_fold_host: the host
restatement of the folded top on the sequential executor) at the project's bar, 1e-9 |ref| + 1e-12.  That emulator runs
the host form of the very fold under test: the independent check is the byte comparison with the knob.  Every case says which
form it expects (spicey_top_fold_form of the handle, and the plan's own decision on the CPU): diode_chain(511) is the
smallest chain that takes the fold (a top of 33 rows, row 0 with a single pivot), diode_chain(766) has a top of 63 rows and
T - 1 row records at level 0, diode_chain(1000) a top of 64 and T (found on the CPU, tests/top_fold_host)."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist
from test_gpu_parity import tol_ratio
from test_packed_resident_gpu import _switched_ladder
from test_top_regs_gpu import _half_clamped_chain
from top_fold_host import pytf

pytestmark = pytest.mark.gpu

STEPS = 64
T = 512
KNOB = "SPICEY_NO_TOP_FOLD"
OTHER_KNOBS = ("SPICEY_NO_U0_RESIDENT", "SPICEY_NO_TOP_REGS", "SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH",
               "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL", "SPICEY_FRESH_FILL_LINEAR")


def _chain(n, seeds=(1, 2), kind="diode_chain"):
    flat, dt, total, src = synth.chain_batch(kind, n, list(seeds), tran=f".tran 1e-6 {(STEPS + 6) * 1e-6:.6g}")
    assert total >= STEPS
    return flat, dt, src[: STEPS + 1]


def _run(flat, dt, src, runs=1, **options):
    """-> (results of `runs` consecutive runs of STEPS steps, info(), spicey_top_fold_form for such a run) of a fresh handle"""
    from spicey_amd.lib import Handle
    h = Handle(flat, **options)
    try:
        form = h.top_fold_form(STEPS)
        r = [h.run(STEPS, dt, src) for _ in range(runs)]
        return r, h.info(), form
    finally:
        h.close()


def _both(monkeypatch, flat, dt, src, want, runs=1, **options):
    """Knob set (the level below the top runs as a phase of its own), knob not set (folded where the plan says so): what
    each handle reports, and the same plan otherwise."""
    options.setdefault("geometry", 2)
    for k in OTHER_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(KNOB, "1")
    off, info_off, form_off = _run(flat, dt, src, runs, **options)
    p_off = pytf.plan(flat, steps=STEPS, **options)
    monkeypatch.delenv(KNOB)
    on, info_on, form_on = _run(flat, dt, src, runs, **options)
    p_on = pytf.plan(flat, steps=STEPS, **options)
    assert info_on == info_off  # the same plan, the same LDS: the knob picks between two kernels of one shape
    assert form_off is False and p_off["rc"] == 0 and (p_off["top_fold"], p_off["top_fold_run"]) == (0, 0)
    assert form_on is bool(want) and p_on["rc"] == 0 and (p_on["top_fold"], p_on["top_fold_run"]) == (int(want), int(want)), (form_on, p_on)
    return off, on, p_on


def _same(off, on, what):
    assert on["status"] == off["status"] and on["detail"] == off["detail"], what
    assert np.array_equal(on["inst_status"], off["inst_status"]), what
    for k in ("out_v", "out_i"):
        assert on[k].tobytes() == off[k].tobytes(), (what, k)
    assert np.array_equal(on["iters"], off["iters"]), (what, "iters")
    if on["status"] == 0:
        assert on["solves"] == off["solves"], what
        for k, v in off["state"].items():
            assert np.asarray(v).tobytes() == np.asarray(on["state"][k]).tobytes(), (what, "state", k)


def _meets_emulator(got, flat, dt, src, fold, what):
    ref = pytf.run(flat, STEPS, dt, src, fold=fold)
    assert ref["status"] == 0 and ref["pcr_n"] > 0
    rv = float(tol_ratio(got["out_v"], ref["out_v"]).max())
    ri = float(tol_ratio(got["out_i"], ref["out_i"]).max())
    print(f"top-fold ratio {what}: out_v {rv:.3g} out_i {ri:.3g} of the bar")
    assert rv <= 1.0 and ri <= 1.0, (what, rv, ri)
    assert np.array_equal(got["iters"], ref["iters"]), what


# chain length -> (the plan takes the fold, rows of the top)
CHAINS = {511: (True, 33), 766: (True, 63), 1000: (True, 64)}


@pytest.mark.parametrize("n", sorted(CHAINS))
def test_a_chain_gives_the_bytes_of_the_unfolded_kernel(n, monkeypatch):
    want, rows = CHAINS[n]
    flat, dt, src = _chain(n)
    off, on, plan = _both(monkeypatch, flat, dt, src, want)
    assert plan["pcr_n"] == rows and (plan["packed"], plan["threads"]) == (1, T)
    assert on[0]["status"] == 0, on[0]["detail"]
    assert np.isfinite(on[0]["out_v"]).all() and np.isfinite(on[0]["out_i"]).all() and float(np.abs(on[0]["out_v"]).max()) > 1.0
    _same(off[0], on[0], n)
    _meets_emulator(on[0], flat, dt, src, want, f"diode_chain({n})")


def test_a_second_run_on_the_handle_and_a_switched_ladder(monkeypatch):
    """Two runs on one handle (the second starts from the first one's end state; the prologue copies the table again), on the
    ladder whose switches make B, the factor phases and the top run several times in a step; 4 instances."""
    flat, dt, src = _switched_ladder()
    src = src[: STEPS + 1]
    off, on, plan = _both(monkeypatch, flat, dt, src, True, runs=2)
    assert on[0]["status"] == 0 and on[1]["status"] == 0
    assert flat.nS > 0 and int(on[0]["iters"].max()) > 1
    _same(off[0], on[0], "switched ladder")
    _same(off[1], on[1], "switched ladder, second run")
    assert not np.array_equal(on[0]["out_v"], on[1]["out_v"])
    _meets_emulator(on[0], flat, dt, src, True, "switched ladder")


def test_three_instances_with_their_own_sources_and_parameters(monkeypatch):
    flat, dt, src = _chain(1000, seeds=(3, 4, 5))
    per = np.ascontiguousarray(np.stack([src * s for s in (1.0, 0.6, -0.4)]))  # (a bipolar one among them: the diodes stay off)
    assert per.shape == (3, STEPS + 1, flat.nV) and not np.array_equal(flat.R_val[0], flat.R_val[1])
    off, on, plan = _both(monkeypatch, flat, dt, per, True)
    assert on[0]["status"] == 0
    _same(off[0], on[0], "three instances")
    assert not np.array_equal(on[0]["out_v"][0], on[0]["out_v"][1]) and not np.array_equal(on[0]["out_v"][1], on[0]["out_v"][2])
    _meets_emulator(on[0], flat, dt, per, True, "three instances, per-instance sources")


def test_a_singular_pivot_is_reported_the_same_way(monkeypatch):
    """Instance 1 of three has node 501 of a 1000-node chain cut off (its resistors 1e16 ohm, its capacitor 1e-30 F, no
    diode there): a pivot of ~2e-16, below the 1e-15 of the reference — an error return, not a fault.  Both forms must name
    the same instance, step and iteration, and the instances beside it must finish with the same bytes."""
    flat, dt, src = _half_clamped_chain(1000)
    node = 501
    assert node not in set(flat.D_np) | set(flat.D_nm) | set(flat.V_n1) | set(flat.V_n2)
    flat.R_val[1, (flat.R_n1 == node) | (flat.R_n2 == node)] = 1e16
    flat.C_val[1, (flat.C_n1 == node) | (flat.C_n2 == node)] = 1e-30
    per = np.ascontiguousarray(np.broadcast_to(src, (3, STEPS + 1, flat.nV)))  # (per-instance layout: partial results stand)
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
    # a plan without the register-exchange top: that form's parent runs, this one does not
    monkeypatch.setenv("SPICEY_NO_TOP_REGS", "1")
    tr, info, form = _run(flat, dt, src, geometry=2)
    assert form is False and info["operand_addr"] == 1 and tr[0]["status"] == 0
    monkeypatch.delenv("SPICEY_NO_TOP_REGS")
    # a linear circuit (factor reuse) keeps the default program
    lin_flat, lin_dt, lin_src = _chain(1000, kind="rc_ladder")
    ln, info, form = _run(lin_flat, lin_dt, lin_src, geometry=2)
    assert form is False and info["factor_reuse"] == 1 and ln[0]["status"] == 0
    # a mesh has no tridiagonal top
    ckt = parseNetlist(synth.rcd_mesh(12, tran=f".tran 1e-6 {(STEPS + 6) * 1e-6:.6g}"))
    mdt, total = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    mesh = abi.flatten(ckt).replicate(2)
    ms, info, form = _run(mesh, mdt, abi.source_table(ckt, mdt, total)[: STEPS + 1], geometry=2)
    assert form is False and info["geometry"] == 2 and ms[0]["status"] == 0
    # a run beyond the ready-argument kernel's step range has no such form (asked of the handle, not run)
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=2)
    try:
        assert h.top_fold_form(STEPS) is True and h.top_fold_form(2**32 - 1) is False
    finally:
        h.close()
    # ... and the packed runs computed the same circuit bit for bit
    assert tr[0]["out_v"].tobytes() == on[0]["out_v"].tobytes() and tr[0]["out_i"].tobytes() == on[0]["out_i"].tobytes() and np.array_equal(tr[0]["iters"], on[0]["iters"])
