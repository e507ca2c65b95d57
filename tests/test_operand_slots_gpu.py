"""Operand-slot kernels (tran_v2_phases.h: OS — ground resolved to a +0.0 slot in Z's resident terminal indices, Z's result
stores on per-section bases, row bases from the phase table, B's empty descriptor fields resolved to a -0.0 slot) on the
GPU against the same shape's early-prefetch kernels: every case runs with SPICEY_NO_OPERAND_SLOTS set and without it and
must give the same bits — voltages, currents, iteration counts, end state — and the run without the knob is held against
the oracle at the project's bar.  33 steps and two instances unless a case says otherwise."""
from __future__ import annotations

import numpy as np
import pytest

from batch_variants import instance
from slots_host import circuits, pyslots
from test_early_prefetch_gpu import _against_oracle, _chain, _mesh34, _run, _same_bits, _switched, _three_sources

pytestmark = pytest.mark.gpu

STEPS = 33
KNOB = "SPICEY_NO_OPERAND_SLOTS"


def _reversed():
    flat, dt, total, src = circuits.reversed_chain(200, n_inst=2, both_grounds=True, tran=".tran 1e-6 4e-5")
    assert total >= STEPS
    return flat, dt, src[: STEPS + 1], STEPS


def _dense():
    flat, dt, total, src = circuits.dense_rows(200, n_inst=2, tran=".tran 1e-6 4e-5")
    assert total >= STEPS
    return flat, dt, src[: STEPS + 1], STEPS


# name: (circuit, geometry, the plan must take the packed fresh shape — the one with operand-slot kernels)
CASES = {
    "diode_chain_1000": (lambda: _chain("diode_chain", 1000), 2, True),   # the bench build
    "diode_chain_100": (lambda: _chain("diode_chain", 100), 2, True),     # most threads own no item: every index names the +0.0 slot
    "diode_chain_333": (lambda: _chain("diode_chain", 333), 2, True),     # counts that are no multiple of a wave or of the workgroup
    "diode_chain_1023": (lambda: _chain("diode_chain", 1023), 2, True),   # the largest chain of the shape: every resident item exists
    "reversed_chain": (_reversed, 2, True),                               # ground as terminal a, and an element between two grounds
    "dense_rows": (_dense, 2, True),                                      # rows of four contributions, entries of two conductances, B's list forms beside them
    "switched_ladder": (_switched, 2, True),                              # nS > 0: Z's switch loop beside the resident section
    "three_sources": (_three_sources, 2, True),
    "rcd_mesh_34": (_mesh34, 0, False),                                   # > 2 x 512 resistors: the beyond-capacity loops keep volt16 / dv16
    "rc_ladder_100": (lambda: _chain("rc_ladder", 100), 0, False),        # linear: factor reuse, the default program
    "one_step": (lambda: _chain("diode_chain", 100, steps=1), 2, True),   # row 0 and row 1 only
}


def _both(monkeypatch, flat, dt, src, steps, geometry, runs=1):
    monkeypatch.delenv("SPICEY_NO_EARLY_PREFETCH", raising=False)
    monkeypatch.setenv(KNOB, "1")
    off, info_off = _run(flat, dt, src, steps, geometry, runs)
    monkeypatch.delenv(KNOB)
    on, info_on = _run(flat, dt, src, steps, geometry, runs)
    assert info_on == info_off  # the same plan, the same LDS: the knob picks between two kernels of one shape
    return off, on, info_on


@pytest.mark.parametrize("case", sorted(CASES))
def test_knob_off_and_on_give_the_same_bits_and_the_oracles_values(case, oracle_backend, monkeypatch):
    make, geometry, packed_fresh = CASES[case]
    flat, dt, src, steps = make()
    off, on, info = _both(monkeypatch, flat, dt, src, steps, geometry)
    if packed_fresh:
        assert info["geometry"] == 2 and info["threads"] == 512 and info["resident_slots"] == 4
        assert pyslots.plan(flat, geometry=geometry)["slots"] == 1  # (the plan of such a handle: the run without the knob took the operand-slot kernel)
    _same_bits(off[0], on[0], case)
    if case == "switched_ladder":
        assert flat.nS > 0 and int(on[0]["iters"].max()) > 1
    if case == "reversed_chain":
        assert (np.asarray(flat.D_np) == 0).all() and float(np.abs(on[0]["out_i"][..., -flat.nD:]).max()) > 1e-6  # the diodes conduct
    j = flat.n_inst - 1
    _against_oracle(oracle_backend, on[0], instance(flat, j), j, steps, dt, src, flat.nS > 0)


def test_two_runs_on_one_handle(oracle_backend, monkeypatch):
    """The second run starts from the first one's end state; its prologue writes the slots and the row bases again."""
    flat, dt, src, steps = _chain("diode_chain", 333)
    off, on, _ = _both(monkeypatch, flat, dt, src, steps, 2, runs=2)
    for r in (0, 1):
        _same_bits(off[r], on[r], f"run {r}")
    assert not np.array_equal(on[0]["out_v"], on[1]["out_v"])  # (the state did carry over)
    j = 1
    ref0 = _against_oracle(oracle_backend, on[0], instance(flat, j), j, steps, dt, src, False)
    nxt = instance(flat, j)
    for k in ("C_vprev", "L_iprev", "D_vdprev"):
        setattr(nxt, k, np.array(ref0["state"][k], dtype=np.float64).reshape(getattr(nxt, k).shape))
    _against_oracle(oracle_backend, on[1], nxt, j, steps, dt, src, False)
