"""Ready-argument kernel (tran_v2_run.h: RA — Z and the early fetch move only their hot arguments to scalars and read the
rest inside the branch that needs it; the record, the source table and the iteration counts come from pointers that the
prologue made the instance's own; step x row is a 32 x 32 -> 64-bit product) on the GPU against the same shape's
operand-slot kernel: every case runs with SPICEY_NO_READY_ARGS set and without it and must give the same bits — voltages,
currents, iteration counts, end state — and the run without the knob is held against the oracle at the project's bar.
33 steps and two instances unless a case says otherwise."""
from __future__ import annotations

import numpy as np
import pytest

from batch_variants import instance
from ready_host import pyready
from spicey_amd import abi
from spicey_amd.netlist import parseNetlist
from test_early_prefetch_gpu import _against_oracle, _chain, _mesh34, _run, _same_bits, _switched, _three_sources

pytestmark = pytest.mark.gpu

STEPS = 33
KNOB = "SPICEY_NO_READY_ARGS"


def _three_instances_own_sources():
    """Three instances, each driven by a source table of its own: src_stride != 0, instance != 0."""
    flat, dt, src, steps = _chain("diode_chain", 200, seeds=(1, 2, 3))
    per = np.stack([src * (1.0 + 0.15 * g) for g in range(flat.n_inst)])
    assert per.shape == (3, steps + 1, flat.nV)
    return flat, dt, per, steps


def _inductor_chain(n=300):
    """A diode chain in which every fifth link is an inductor.  (The packed shape takes no circuit with more than 2 x 512
    elements of a kind — spicey_plan refuses geometry 2 for two parallel resistors per link of a 520-node chain —, so of Z's
    beyond-capacity loops it can only run those that have no resident form: inductors and switches.  The inductor loop is
    the one that reads the static conductances through the base formed inside the cold branch, and L_iprev on the last step.)"""
    L = ["* chain with inductors", ".model DM D(Is=1e-14 N=1)", "V1 n1 0 PULSE(0 5 0 1e-6 1e-6 4e-6 1e-5)"]
    for k in range(1, n):
        if k % 5 == 0: L.append(f"L{k} n{k} n{k+1} {1e-6 * (1 + 0.01 * (k % 7)):.6g}")
        else: L.append(f"R{k} n{k} n{k+1} {100 * (1 + 0.001 * (k % 17)):.6g}")
        L.append(f"C{k} n{k+1} 0 {1e-9 * (1 + 0.002 * (k % 11)):.6g}")
        if k % 2: L.append(f"D{k} n{k+1} 0 DM")
    L += [".tran 1e-6 4e-5", ".end", ""]
    ckt = parseNetlist("\n".join(L))
    dt, total = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    flat = abi.flatten(ckt).replicate(2)
    flat.R_val[1] *= 1.02
    flat.L_val[1] *= 0.97
    assert flat.nL > 0 and total >= STEPS
    return flat, dt, abi.source_table(ckt, dt, total)[: STEPS + 1], STEPS


# name: (circuit, geometry, the plan must take the ready-argument kernel)
CASES = {
    "diode_chain_100": (lambda: _chain("diode_chain", 100), 2, True),     # most threads own no item
    "diode_chain_333": (lambda: _chain("diode_chain", 333), 2, True),     # counts that are no multiple of a wave
    "diode_chain_1023": (lambda: _chain("diode_chain", 1023), 2, True),   # every resident item exists
    "three_sources": (_three_sources, 2, True),                           # nV > 1: source base plus lane
    "own_sources": (_three_instances_own_sources, 2, True),               # src_stride != 0, instance != 0
    "switched_ladder": (_switched, 2, True),                              # re-iteration, Z's switch loop beside lazily fetched arguments
    "inductor_chain": (_inductor_chain, 2, True),                         # a beyond-capacity loop's own fetches
    "one_step": (lambda: _chain("diode_chain", 100, steps=1), 2, True),   # the first step is also the last
    "rcd_mesh_34": (_mesh34, 0, False),                                   # the plan says no, and the parent's kernel runs
}


def _both(monkeypatch, flat, dt, src, steps, geometry, runs=1):
    for k in ("SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_OPERAND_SLOTS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(KNOB, "1")
    off, info_off = _run(flat, dt, src, steps, geometry, runs)
    monkeypatch.delenv(KNOB)
    on, info_on = _run(flat, dt, src, steps, geometry, runs)
    assert info_on == info_off  # the same plan, the same LDS: the knob picks between two kernels of one shape
    return off, on, info_on


@pytest.mark.parametrize("case", sorted(CASES))
def test_knob_off_and_on_give_the_same_bits_and_the_oracles_values(case, oracle_backend, monkeypatch):
    make, geometry, ready = CASES[case]
    flat, dt, src, steps = make()
    off, on, info = _both(monkeypatch, flat, dt, src, steps, geometry)
    p = pyready.plan(flat, steps=steps, geometry=geometry)  # (the plan of such a handle, and what this run launched)
    assert p["rc"] == 0 and p["ready_run"] == int(ready)
    if ready:
        assert info["geometry"] == 2 and info["threads"] == 512 and info["resident_slots"] == 4
    _same_bits(off[0], on[0], case)
    if case == "switched_ladder":
        assert flat.nS > 0 and int(on[0]["iters"].max()) > 1
    if case == "three_sources":
        assert flat.nV == 3
    j = flat.n_inst - 1
    _against_oracle(oracle_backend, on[0], instance(flat, j), j, steps, dt, src[j] if np.ndim(src) == 3 else src, flat.nS > 0)


def _run_plain(flat, dt, src, steps, **kw):
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=2)
    try:
        r = h.run(steps, dt, src, **kw)
        assert r["status"] == 0, r["detail"]
        return r
    finally:
        h.close()


def test_a_run_without_currents(oracle_backend, monkeypatch):
    """A null current pointer stays null through the rebasing; voltages, counts and end state are those of the full run."""
    flat, dt, src, steps = _chain("diode_chain", 333)
    monkeypatch.delenv(KNOB, raising=False)
    assert pyready.plan(flat, steps=steps, geometry=2)["ready_run"] == 1
    got = _run_plain(flat, dt, src, steps, want_currents=False)
    monkeypatch.setenv(KNOB, "1")
    off = _run_plain(flat, dt, src, steps, want_currents=False)
    assert got["out_i"] is None and off["out_i"] is None
    assert np.array_equal(got["out_v"], off["out_v"]) and np.array_equal(got["iters"], off["iters"])
    for k, v in off["state"].items():
        assert np.array_equal(np.asarray(v), np.asarray(got["state"][k])), k
    ref = oracle_backend.run(instance(flat, 1), steps, dt, src)
    from test_gpu_parity import tol_ratio
    assert tol_ratio(got["out_v"][1], ref["out_v"][0]).max() <= 1.0


def _two_runs(flat, dt, src, first, second):
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=2)
    try:
        a = h.run(first, dt, src[: first + 1])
        b = h.run(second, dt, src[: second + 1])
        assert a["status"] == 0 and b["status"] == 0, (a["detail"], b["detail"])
        return a, b
    finally:
        h.close()


def test_two_runs_of_different_length_on_one_handle(oracle_backend, monkeypatch):
    """The second run starts from the first one's end state — written through the last step's lazily read pointers — and its
    prologue rebuilds the bases for its own step count."""
    flat, dt, src, steps = _chain("diode_chain", 333)
    first, second = steps, 17
    monkeypatch.setenv(KNOB, "1")
    off = _two_runs(flat, dt, src, first, second)
    monkeypatch.delenv(KNOB)
    on = _two_runs(flat, dt, src, first, second)
    for r in (0, 1):
        _same_bits(off[r], on[r], f"run {r}")
    assert on[1]["out_v"].shape[1] == second + 1 and not np.array_equal(on[0]["out_v"][:, : second + 1], on[1]["out_v"])  # (the state did carry over)
    j = 1
    ref0 = _against_oracle(oracle_backend, on[0], instance(flat, j), j, first, dt, src[: first + 1], False)
    nxt = instance(flat, j)
    for k in ("C_vprev", "L_iprev", "D_vdprev"):
        setattr(nxt, k, np.array(ref0["state"][k], dtype=np.float64).reshape(getattr(nxt, k).shape))
    _against_oracle(oracle_backend, on[1], nxt, j, second, dt, src[: second + 1], False)
