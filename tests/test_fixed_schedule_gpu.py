"""The fixed schedule (tran_v2_run.h: FS — the fused packed kernel with its time loop written out for what the plan holds, an
executor without profiling code, the iteration counts written once behind the loop) on the GPU.

Every case runs on the packed layout (512 threads, 4 slots), 64 steps unless it says otherwise, with
SPICEY_NO_FIXED_SCHEDULE and without, on fresh handles, and must give the same bytes — voltages, currents, iteration
counts, status, detail, per-instance status, solve count, end state.  Every case says which form it expects
(spicey_fixed_schedule_form of the handle, and the plan's own decision on the CPU, tests/fixed_schedule_host).
diode_chain(511) is the smallest chain that takes the form, (1000) the bench circuit, (1018) the largest; (766) and (1022)
take the fuse but stream a second phase beside level 0, which the written-out loop has no path for: the plan refuses the
form there (tests/test_fixed_schedule.py) and both handles run the fused kernel of today."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import abi, synth
from test_packed_resident_gpu import _switched_ladder
from test_stamp_fuse import chain_with_inductor, _from_text
from test_top_regs_gpu import _half_clamped_chain
from test_fixed_schedule import singular_later
from fixed_schedule_host import pyfs

pytestmark = pytest.mark.gpu

STEPS = 64
T = 512
KNOB = "SPICEY_NO_FIXED_SCHEDULE"
OTHER_KNOBS = ("SPICEY_NO_STAMP_FUSE", "SPICEY_NO_TOP_FOLD", "SPICEY_NO_U0_RESIDENT", "SPICEY_NO_TOP_REGS", "SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS",
               "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL", "SPICEY_FRESH_FILL_LINEAR", "SPICEY_NO_KMERGE")
TRAN = f".tran 1e-6 {(STEPS + 6) * 1e-6:.6g}"
SENTINEL = -7


def _chain(n, seeds=(1, 2), kind="diode_chain"):
    flat, dt, total, src = synth.chain_batch(kind, n, list(seeds), tran=TRAN)
    assert total >= STEPS
    return flat, dt, src[: STEPS + 1]


def _run(flat, dt, src, runs=1, steps=STEPS, currents=True, **options):
    """-> (results of `runs` consecutive runs of `steps` steps, info(), spicey_fixed_schedule_form for such a run) of a fresh handle"""
    from spicey_amd.lib import Handle
    h = Handle(flat, **options)
    try:
        form = h.fixed_schedule_form(steps)
        r = [h.run(steps, dt, src[: steps + 1] if src.ndim < 3 else src[:, : steps + 1], want_currents=currents) for _ in range(runs)]
        return r, h.info(), form
    finally:
        h.close()


def _both(monkeypatch, flat, dt, src, want, runs=1, steps=STEPS, currents=True, **options):
    """Knob set (the loop decides its schedule in every step), knob not set (the written-out loop where the plan says so): what
    each handle reports, and the same plan otherwise."""
    options.setdefault("geometry", 2)
    for k in OTHER_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(KNOB, "1")
    off, info_off, form_off = _run(flat, dt, src, runs, steps, currents, **options)
    p_off = pyfs.plan(flat, steps=steps, **{k: v for k, v in options.items() if k != "profile"})
    monkeypatch.delenv(KNOB)
    on, info_on, form_on = _run(flat, dt, src, runs, steps, currents, **options)
    p_on = pyfs.plan(flat, steps=steps, **{k: v for k, v in options.items() if k != "profile"})
    assert info_on == info_off  # the same plan, the same LDS: the knob picks between two kernels of one shape
    assert form_off is False and p_off["rc"] == 0 and (p_off["fixed_schedule"], p_off["fixed_schedule_run"]) == (0, 0)
    assert form_on is bool(want) and p_on["rc"] == 0 and (p_on["fixed_schedule"], p_on["fixed_schedule_run"]) == (int(want), int(want)), (form_on, p_on)
    assert p_on["stamp_fuse_run"] == p_off["stamp_fuse_run"]  # (the knob leaves the fuse alone)
    return off, on, p_on


def _same(off, on, what):
    assert on["status"] == off["status"] and on["detail"] == off["detail"], what
    assert np.array_equal(on["inst_status"], off["inst_status"]), what
    for k in ("out_v", "out_i"):
        assert (on[k] is None) == (off[k] is None), (what, k)
        if on[k] is not None:
            assert on[k].tobytes() == off[k].tobytes(), (what, k)
    assert on["iters"].tobytes() == off["iters"].tobytes(), (what, "iters")
    if on["status"] == 0:
        assert on["solves"] == off["solves"], what
        for k, v in off["state"].items():
            assert np.asarray(v).tobytes() == np.asarray(on["state"][k]).tobytes(), (what, "state", k)


@pytest.mark.parametrize("n,takes", [(511, True), (766, False), (1000, True), (1018, True), (1022, False)])
def test_a_chain_gives_the_bytes_of_the_kernel_that_decides_in_every_step(n, takes, monkeypatch):
    flat, dt, src = _chain(n)
    off, on, plan = _both(monkeypatch, flat, dt, src, takes)
    assert (plan["packed"], plan["threads"], plan["stamp_fuse_run"]) == (1, T, 1)
    assert on[0]["status"] == 0, on[0]["detail"]
    assert np.isfinite(on[0]["out_v"]).all() and np.isfinite(on[0]["out_i"]).all() and float(np.abs(on[0]["out_v"]).max()) > 1.0
    assert (on[0]["iters"] == 1).all()
    _same(off[0], on[0], n)


def test_a_second_run_on_the_handle(monkeypatch):
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


def test_a_run_without_currents(monkeypatch):
    flat, dt, src = _chain(1000)
    off, on, plan = _both(monkeypatch, flat, dt, src, True, currents=False)
    assert on[0]["status"] == 0 and on[0]["out_i"] is None
    _same(off[0], on[0], "no currents")


def test_a_run_of_one_step(monkeypatch):
    flat, dt, src = _chain(1000)
    off, on, plan = _both(monkeypatch, flat, dt, src, True, steps=1)
    assert on[0]["status"] == 0 and on[0]["out_v"].shape[1] == 2 and (on[0]["iters"] == 1).all()
    _same(off[0], on[0], "one step")


def test_the_folds_singular_instance_is_reported_the_same_way(monkeypatch):
    """The singular instance of the fold's test: instance 1 of three has node 501 of the half-clamped 1000-node chain cut off.
    That chain has no fuse, so the plan refuses the form: both handles run today's kernel and name the same instance and step."""
    flat, dt, src = _half_clamped_chain(1000)
    node = 501
    assert node not in set(flat.D_np) | set(flat.D_nm) | set(flat.V_n1) | set(flat.V_n2)
    flat.R_val[1, (flat.R_n1 == node) | (flat.R_n2 == node)] = 1e16
    flat.C_val[1, (flat.C_n1 == node) | (flat.C_n2 == node)] = 1e-30
    per = np.ascontiguousarray(np.broadcast_to(src, (3, STEPS + 1, flat.nV)))
    off, on, plan = _both(monkeypatch, flat, dt, per, False)
    on, off = on[0], off[0]
    assert on["status"] == abi.ERR_SINGULAR and "singular at inst 1 step 0" in on["detail"]
    assert np.array_equal(on["inst_status"], [0, abi.ERR_SINGULAR, 0])
    _same(off, on, "the fold's singular instance")


def _run_on_device_buffers(flat, dt, per, steps=STEPS, **options):
    """One run through run_device on buffers of the test's own (the HIP runtime the library links: test_exact_order_gpu._hip),
    the iteration counts filled with SENTINEL before the launch: -> (spicey_sync's status, per-instance status, detail, out_v,
    out_i, the counts as the kernel left them, form)"""
    import ctypes as C
    from spicey_amd.lib import Handle
    from test_exact_order_gpu import _hip
    H = _hip()
    ni, np1 = flat.n_inst, steps + 1
    per = np.ascontiguousarray(per, dtype=np.float64)
    ov, oi = np.zeros((ni, np1, flat.n_out)), np.zeros((ni, np1, flat.n_cur))
    it = np.full((ni, np1), SENTINEL, np.int32)
    host = {"src": per, "ov": ov, "oi": oi, "it": it}
    d = {k: C.c_void_p() for k in host}
    h = Handle(flat, **options)
    try:
        form = h.fixed_schedule_form(steps)
        for k, a in host.items():
            assert H.hipMalloc(C.byref(d[k]), a.nbytes) == 0
            assert H.hipMemcpy(d[k], a.ctypes.data, a.nbytes, 1) == 0  # host to device
        h.run_device(steps, dt, d["src"].value, d["ov"].value, d["oi"].value, d["it"].value, src_per_inst=True)
        rc = h.sync()
        for k in ("ov", "oi", "it"):
            assert H.hipMemcpy(host[k].ctypes.data, d[k], host[k].nbytes, 2) == 0  # device to host
        return rc, h.inst_status(), h.error(), ov, oi, it, form
    finally:
        h.close()
        for v in d.values():
            if v.value:
                H.hipFree(v)


def test_a_pivot_that_turns_singular_at_a_later_step(monkeypatch):
    """A chain that takes the form, whose instance 1 turns singular at a step > 0 (test_fixed_schedule.singular_later).  Status,
    detail, error step and every byte must match the knob's; and with the iteration counts filled with a sentinel before the
    launch, no entry at or behind the error step may be written — on either kernel."""
    flat, dt, per = singular_later(STEPS)
    off, on, plan = _both(monkeypatch, flat, dt, per, True)
    on, off = on[0], off[0]
    assert on["status"] == abi.ERR_SINGULAR and np.array_equal(on["inst_status"], [0, abi.ERR_SINGULAR, 0])
    assert "singular at inst 1 step " in on["detail"]
    _same(off, on, "singular at a later step")
    step = int(on["detail"].split("step ")[1].split()[0])
    assert 0 < step <= STEPS
    monkeypatch.setenv(KNOB, "1")
    rc0, st0, det0, v0, i0, it0, form0 = _run_on_device_buffers(flat, dt, per, geometry=2)
    monkeypatch.delenv(KNOB)
    rc1, st1, det1, v1, i1, it1, form1 = _run_on_device_buffers(flat, dt, per, geometry=2)
    assert (form0, form1) == (False, True)
    assert rc1 == rc0 == abi.ERR_SINGULAR and det1 == det0 and f"step {step} " in det1 + " " and np.array_equal(st1, st0)
    assert (it1[0] == 1).all() and (it1[2] == 1).all() and (it1[1][:step] == 1).all() and (it1[1][step:] == SENTINEL).all()
    assert it1.tobytes() == it0.tobytes() and v1.tobytes() == v0.tobytes() and i1.tobytes() == i0.tobytes()


def test_the_kernel_with_phase_timers_gives_the_bytes_of_the_production_kernel(monkeypatch):
    """profile = 1 launches the form's second kernel, built with the profiling executor: the same bytes, and a phase table."""
    from spicey_amd.lib import Handle
    for k in OTHER_KNOBS + (KNOB,):
        monkeypatch.delenv(k, raising=False)
    flat, dt, src = _chain(1000)
    plain, _, form = _run(flat, dt, src, geometry=2)
    assert form is True and plain[0]["status"] == 0
    h = Handle(flat, geometry=2, profile=True)
    try:
        assert h.fixed_schedule_form(STEPS) is True
        timed = h.run(STEPS, dt, src, want_currents=True)
        prof = h.phase_cycles()
    finally:
        h.close()
    _same(plain[0], timed, "phase timers")
    # Z, its second phase (A's slot), U_0, K_0 were timed — and the time loop holds no phase B
    assert prof["Z"] > 0 and prof["A"] > 0 and prof["U"][0] > 0 and prof["K"][0] > 0 and prof["run_cycles"] > 0


def test_the_form_is_not_taken_where_its_conditions_fail(monkeypatch):
    for k in OTHER_KNOBS + (KNOB,):
        monkeypatch.delenv(k, raising=False)
    flat, dt, src = _chain(1000)
    on, _, form = _run(flat, dt, src, geometry=2)
    assert form is True and on[0]["status"] == 0
    # a plan without the fuse: that form's parent runs, this one does not
    monkeypatch.setenv("SPICEY_NO_STAMP_FUSE", "1")
    tr, info, form = _run(flat, dt, src, geometry=2)
    assert form is False and tr[0]["status"] == 0
    monkeypatch.delenv("SPICEY_NO_STAMP_FUSE")
    assert tr[0]["out_v"].tobytes() == on[0]["out_v"].tobytes() and tr[0]["out_i"].tobytes() == on[0]["out_i"].tobytes() and np.array_equal(tr[0]["iters"], on[0]["iters"])
    # empty diagnostics phases: the written-out loop has none
    tr, info, form = _run(flat, dt, src, geometry=2, debug_empty_phases=1)
    assert form is False and tr[0]["status"] == 0 and tr[0]["out_v"].tobytes() == on[0]["out_v"].tobytes()
    refused = {
        "rc_ladder": _chain(1000, kind="rc_ladder"),
        "switched_ladder": (lambda f, d, s: (f, d, s[: STEPS + 1]))(*_switched_ladder()),
        "inductor": chain_with_inductor(steps=STEPS),
        "rcd_mesh": (lambda f, d, s: (f.replicate(2), d, s))(*_from_text(synth.rcd_mesh(12, tran=TRAN), STEPS)),
    }
    for what, (f, d, s) in refused.items():
        assert len(s) == STEPS + 1
        assert pyfs.plan(f, steps=STEPS, geometry=2)["fixed_schedule_run"] == 0, what
        r, info, form = _run(f, d, s, geometry=2)
        assert form is False and r[0]["status"] == 0, (what, r[0]["detail"])
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=2)
    try:
        assert h.fixed_schedule_form(STEPS) is True and h.fixed_schedule_form(2**32 - 1) is False
    finally:
        h.close()
