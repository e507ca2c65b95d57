"""The resident level-0 record (tran_v2_run.h: UR — the packed register-exchange-top kernel whose prologue loads the row
record of factor level 0 into registers once, whose phase B fetches nothing and whose phase 0 runs the registers) and
spicey_exp (tran_common.h: the device library's exp with its constants read from constant memory inside the phase) on the
GPU.

exp: a probe kernel (tests/u0_host/exp_probe.hip, compiled like kernels.hip) evaluates the device library's exp and
spicey_exp on the same doubles — 2^20 arguments over [-45, 35], the clamped junction voltage [-1, 0.8] times 1 / (N VT)
with margin, and the edges of the range tests — and every pair must have the same bits.

Kernel: every case runs on the packed layout (512 threads, 4 slots), 64 steps, all voltages and currents, with
SPICEY_NO_U0_RESIDENT and without, and must give the same bits — voltages, currents, iteration counts, statuses, solve
count, end state; the run without the knob is held against the emulator of this very build (tests/u0_host: the fresh
operand-address build on the sequential executor, in the form the plan takes) at the project's bar, 1e-9 |ref| + 1e-12.
Every case says which form it expects (spicey_u0_resident_form of the handle, and the plan's own decision on the CPU):
diode_chain(22) and diode_chain(100) keep level 0 resident in the slots — no plan takes the form, both runs are one
kernel — diode_chain(1000) has T = 512 row records, diode_chain(766) T - 1 (found on the CPU, tests/u0_host, for
n = 20 .. 1023: 511 records for n = 766 .. 893, 512 for n = 894 .. 1022, 513 — refused — for n = 1023)."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from spicey_amd import abi, synth
from test_gpu_parity import tol_ratio
from test_packed_resident_gpu import _switched_ladder
from test_top_regs_gpu import _half_clamped_chain
from u0_host import pyu0

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 64
T = 512
KNOB = "SPICEY_NO_U0_RESIDENT"
OTHER_KNOBS = ("SPICEY_NO_TOP_REGS", "SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS", "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE",
               "SPICEY_NO_FRESH_FILL", "SPICEY_FRESH_FILL_LINEAR")


def exp_arguments():
    rng = np.random.default_rng(19)
    edges = []
    for v in (0.0, -0.0, np.inf, -np.inf, np.nan, 709.78, 1024.0, 1025.0, -745.0, -1075.0, -1076.0, -45.0, 35.0):
        edges.append(v)
    for v in (709.78, 1024.0, 1025.0, -745.0, -1075.0, -1076.0, 709.782712893384, -745.1332191019411, -708.3964185322641):  # (+ libm's overflow, underflow and subnormal thresholds)
        edges += [np.nextafter(v, np.inf), np.nextafter(v, -np.inf), v]
    return np.concatenate([np.linspace(-45.0, 35.0, 1 << 19), rng.uniform(-45.0, 35.0, 1 << 19), np.array(edges)])


def test_spicey_exp_has_the_bits_of_the_device_librarys_exp(tmp_path):
    exe = str(tmp_path / "exp_probe")
    src = os.path.join(REPO, "tests", "u0_host", "exp_probe.hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", exe, src], check=True, timeout=300)
    x = exp_arguments()
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    x.astype(np.float64).tofile(inp)
    subprocess.run([exe, inp, outp], check=True, timeout=120)
    got = np.fromfile(outp, np.float64)
    assert got.size == 2 * x.size
    lib, port = got[: x.size], got[x.size:]
    bad = lib.view(np.uint64) != port.view(np.uint64)
    print(f"exp against spicey_exp on {x.size} arguments: {int(bad.sum())} pairs differ")
    assert not bad.any(), (x[bad][:5], lib[bad][:5], port[bad][:5])
    # (and the probe did evaluate something: exp(0) = 1, exp(1024+) = inf, exp(-1076) = 0, NaN stays NaN)
    assert lib[x == 0.0].tolist() == [1.0, 1.0] and np.isinf(lib[x == 1025.0]).all() and (lib[x == -1076.0] == 0.0).all() and np.isnan(lib[np.isnan(x)]).all()
    assert abs(lib[1 << 18] / np.exp(x[1 << 18]) - 1.0) < 1e-15


def _chain(n, seeds=(1, 2)):
    flat, dt, total, src = synth.chain_batch("diode_chain", n, list(seeds), tran=f".tran 1e-6 {(STEPS + 6) * 1e-6:.6g}")
    assert total >= STEPS
    return flat, dt, src[: STEPS + 1]


def _run(flat, dt, src, runs=1, **options):
    """-> (results of `runs` consecutive runs of STEPS steps, info(), spicey_u0_resident_form for such a run) of a fresh handle"""
    from spicey_amd.lib import Handle
    h = Handle(flat, **options)
    try:
        form = h.u0_resident_form(STEPS)
        r = [h.run(STEPS, dt, src) for _ in range(runs)]
        return r, h.info(), form
    finally:
        h.close()


def _both(monkeypatch, flat, dt, src, want, runs=1, **options):
    """Knob set (the record is fetched under B in every step), knob not set (resident where the plan says so): what each
    handle reports, and the same plan otherwise."""
    options.setdefault("geometry", 2)
    for k in OTHER_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(KNOB, "1")
    off, info_off, form_off = _run(flat, dt, src, runs, **options)
    p_off = pyu0.plan(flat, steps=STEPS, **options)
    monkeypatch.delenv(KNOB)
    on, info_on, form_on = _run(flat, dt, src, runs, **options)
    p_on = pyu0.plan(flat, steps=STEPS, **options)
    assert info_on == info_off  # the same plan, the same LDS: the knob picks between two kernels of one shape
    assert form_off is False and p_off["rc"] == 0 and (p_off["u0_resident"], p_off["u0_resident_run"]) == (0, 0)
    assert form_on is bool(want) and p_on["rc"] == 0 and (p_on["u0_resident"], p_on["u0_resident_run"]) == (int(want), int(want)), (form_on, p_on)
    assert (info_on["interpreter"], info_on["geometry"], info_on["threads"], info_on["resident_slots"], info_on["operand_addr"]) == (2, 2, T, 4, 1)
    return off, on, p_on


def _same(off, on, what):
    assert on["status"] == off["status"] and on["detail"] == off["detail"], what
    assert np.array_equal(on["inst_status"], off["inst_status"]), what
    for k in ("out_v", "out_i"):
        assert np.array_equal(on[k], off[k], equal_nan=True), (what, k)
    assert np.array_equal(on["iters"], off["iters"]), (what, "iters")
    if on["status"] == 0:
        assert on["solves"] == off["solves"], what
        for k, v in off["state"].items():
            assert np.array_equal(np.asarray(v), np.asarray(on["state"][k]), equal_nan=(k != "S_ison")), (what, "state", k)


def _meets_emulator(got, flat, dt, src, resident, what):
    ref = pyu0.run(flat, STEPS, dt, src, resident=resident)
    assert ref["status"] == 0 and ref["pcr_n"] > 0
    rv = float(tol_ratio(got["out_v"], ref["out_v"]).max())
    ri = float(tol_ratio(got["out_i"], ref["out_i"]).max())
    print(f"u0-resident ratio {what}: out_v {rv:.3g} out_i {ri:.3g} of the bar")
    assert rv <= 1.0 and ri <= 1.0, (what, rv, ri)
    assert np.array_equal(got["iters"], ref["iters"]), what


# chain length -> (the plan takes the form, row records of level 0)
CHAINS = {22: (False, 0), 100: (False, 0), 766: (True, T - 1), 1000: (True, T)}


@pytest.mark.parametrize("n", sorted(CHAINS))
def test_a_chain_gives_the_bits_of_the_fetched_record(n, monkeypatch):
    want, records = CHAINS[n]
    flat, dt, src = _chain(n)
    off, on, plan = _both(monkeypatch, flat, dt, src, want)
    assert (plan["rows"], plan["records"], plan["remainder"]) == (int(want), records, 0)
    assert on[0]["status"] == 0, on[0]["detail"]
    assert np.isfinite(on[0]["out_v"]).all() and np.isfinite(on[0]["out_i"]).all()
    _same(off[0], on[0], n)
    _meets_emulator(on[0], flat, dt, src, want, f"diode_chain({n})")


def test_a_second_run_on_the_handle_and_a_switched_ladder(monkeypatch):
    """Two runs on one handle (the second starts from the first one's end state; the prologue loads the record again), on
    the ladder whose switches make B, the factor phases and the top run several times in a step; 4 instances."""
    flat, dt, src = _switched_ladder()
    src = src[: STEPS + 1]
    off, on, plan = _both(monkeypatch, flat, dt, src, True, runs=2)
    assert on[0]["status"] == 0 and on[1]["status"] == 0
    assert flat.nS > 0 and int(on[0]["iters"].max()) > 1
    _same(off[0], on[0], "switched ladder")
    _same(off[1], on[1], "switched ladder, second run")
    assert not np.array_equal(on[0]["out_v"], on[1]["out_v"])
    _meets_emulator(on[0], flat, dt, src, True, "switched ladder")


def test_three_instances_with_their_own_sources(monkeypatch):
    flat, dt, src = _chain(1000, seeds=(3, 4, 5))
    per = np.ascontiguousarray(np.stack([src * s for s in (1.0, 0.6, -0.4)]))  # (a bipolar one among them: the diodes stay off)
    assert per.shape == (3, STEPS + 1, flat.nV)
    off, on, plan = _both(monkeypatch, flat, dt, per, True)
    assert on[0]["status"] == 0
    _same(off[0], on[0], "three instances")
    assert not np.array_equal(on[0]["out_v"][0], on[0]["out_v"][1]) and not np.array_equal(on[0]["out_v"][1], on[0]["out_v"][2])
    _meets_emulator(on[0], flat, dt, per, True, "three instances, per-instance sources")


def test_a_singular_pivot_below_the_top_is_reported_the_same_way(monkeypatch):
    """Instance 1 of three has node 501 of a 1000-node chain cut off (its resistors 1e16 ohm, its capacitor 1e-30 F, no
    diode there): a pivot of ~2e-16, below the 1e-15 of the reference — an error return, not a fault.  Both forms must name
    the same instance, step and iteration, and the instances beside it must finish with the same bits."""
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
            assert np.array_equal(on[k][j], off[k][j]), (j, k)
        assert np.isfinite(on["out_v"][j]).all()


def test_the_form_is_not_taken_where_its_conditions_fail(monkeypatch):
    for k in OTHER_KNOBS + (KNOB,):
        monkeypatch.delenv(k, raising=False)
    flat, dt, src = _chain(1000)
    # by default on this shape
    on, _, form = _run(flat, dt, src, geometry=2)
    assert form is True and on[0]["status"] == 0
    # the latency geometry has no such kernel
    lat, info, form = _run(flat, dt, src, geometry=1)
    assert form is False and info["geometry"] == 1 and lat[0]["status"] == 0
    # where the condition of the form below it fails, that one's parent runs and this one does not
    monkeypatch.setenv("SPICEY_NO_TOP_REGS", "1")
    tr, info, form = _run(flat, dt, src, geometry=2)
    assert form is False and info["operand_addr"] == 1 and tr[0]["status"] == 0
    monkeypatch.delenv("SPICEY_NO_TOP_REGS")
    # one row record more than threads: the entry point says no, the fetching kernel runs
    long_flat, long_dt, long_src = _chain(1023)
    lg, info, form = _run(long_flat, long_dt, long_src, geometry=2)
    assert form is False and info["geometry"] == 2 and lg[0]["status"] == 0
    # a linear circuit (factor reuse) keeps the default program
    lin_flat, lin_dt, total, lin_src = synth.chain_batch("rc_ladder", 1000, [1, 2], tran=f".tran 1e-6 {(STEPS + 6) * 1e-6:.6g}")
    ln, info, form = _run(lin_flat, lin_dt, lin_src[: STEPS + 1], geometry=2)
    assert form is False and info["factor_reuse"] == 1 and ln[0]["status"] == 0
    # a run beyond the ready-argument kernel's step range has no such form (asked of the handle, not run)
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=2)
    try:
        assert h.u0_resident_form(STEPS) is True and h.u0_resident_form(2**32 - 1) is False
    finally:
        h.close()
    # ... and all of them computed the same circuit: the packed one bit for bit
    assert np.array_equal(tr[0]["out_v"], on[0]["out_v"]) and np.array_equal(tr[0]["out_i"], on[0]["out_i"]) and np.array_equal(tr[0]["iters"], on[0]["iters"])
    assert tol_ratio(lat[0]["out_v"], on[0]["out_v"]).max() <= 1.0
