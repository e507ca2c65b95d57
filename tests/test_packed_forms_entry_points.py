"""Every transient entry point on the packed kernel's fused forms, on the CPU: what tests/test_packed_forms_entry_points_gpu.py
expects of a device, checked first on the plan harnesses (tests/addr_host, tests/top_fold_host, tests/stamp_fuse_host) and on
the emulator of the fused phases (tests/stamp_fuse_host), which is also held against the oracle here so that the reference
side of the GPU tests is honest.

The forms (ready arguments, operand addresses, register-exchange top, resident level-0 record, folded last factor level,
stamp fuse) each came with a test of Handle.run, all voltages recorded, one dt.  The other entry points — a probe filter,
per-instance diode parameters, another dt on the same handle, substituted element values — change exactly what those forms
moved into registers, prologue-built records and host-built tables.  This file defines the circuits, the knob ladder and the
forms every ladder level must report, and checks on the CPU:

  - the plan takes fold and fuse for CHAIN under every probe filter and with per-instance diode parameters, and reports at
    each ladder level the forms the GPU tests assert of the handle (also for LADDER, MESH and the chain with a bare node);
  - the emulator's filtered run is the column selection of its unfiltered run, with a +0.0 column for ground;
  - with per-instance D_is and D_n the fused and the unfused emulator agree in bytes and every instance meets the oracle;
  - a second run at dt / 2, continued from the first run's state, agrees in bytes between the two and meets the oracle
    started from that state;
  - the oracle's v(n64) crosses the threshold the GPU module's when() uses well inside the run.

Bar against the oracle: the project's, |x - ref| <= 1e-9 |ref| + 1e-12, iteration counts identical."""
from __future__ import annotations

import numpy as np
import pytest

from addr_host import pyaddr
from batch_variants import instance
from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist
from stamp_fuse_host import pysf
from test_gpu_parity import tol_ratio
from test_packed_resident_gpu import _switched_ladder
from test_stamp_fuse import _from_text, chain_with_bare_node
from top_fold_host import pytf

STEPS = 64
HALF = STEPS // 2
N = 511  # the smallest diode chain that folds and fuses (tests/test_stamp_fuse.py)
TRAN = ".tran 1e-6 7e-5"
# every knob of tests/test_stamp_fuse_gpu.py (OTHER_KNOBS + (KNOB,)): together they select the oldest packed kernel
ALL = ("SPICEY_NO_TOP_FOLD", "SPICEY_NO_U0_RESIDENT", "SPICEY_NO_TOP_REGS", "SPICEY_NO_OPERAND_ADDR", "SPICEY_NO_READY_ARGS", "SPICEY_NO_OPERAND_SLOTS",
       "SPICEY_NO_EARLY_PREFETCH", "SPICEY_NO_PHASE_TABLE", "SPICEY_NO_FRESH_FILL", "SPICEY_FRESH_FILL_LINEAR", "SPICEY_NO_STAMP_FUSE")
LEVELS = [(), ("SPICEY_NO_STAMP_FUSE",), ("SPICEY_NO_TOP_FOLD",), ("SPICEY_NO_U0_RESIDENT",), ("SPICEY_NO_TOP_REGS",), ("SPICEY_NO_OPERAND_ADDR",),
          ("SPICEY_NO_READY_ARGS",), ALL]
LEVEL_IDS = ["top", "no_stamp_fuse", "no_top_fold", "no_u0_resident", "no_top_regs", "no_operand_addr", "no_ready_args", "all_knobs"]
FILTERS = {"three": [511, 1, 7], "ground_repeat": [0, 5, 511, 5, 300], "reverse": list(range(N, 0, -1))}
WHEN_LEVEL = 0.01  # volts: v(n64) of every CHAIN instance rises through it between steps 8 and 56 (test below)

# what a handle reports at the top of the ladder: (stamp_fuse_form, top_fold_form, u0_resident_form, top_regs_form, info operand_addr)
BASE_FORMS = {"chain": (1, 1, 1, 1, 1),   # folds and fuses
              "ladder": (0, 1, 1, 1, 1),  # nS > 0: the step re-iterates, so no fuse; the fold stays
              "mesh": (0, 0, 0, 0, 0)}    # no tridiagonal top, overflow lists: the early-prefetch fresh-fill kernel on generic streamed records


def expected_forms(base, level: int):
    """The forms of BASE_FORMS a fresh handle must report at LEVELS[level]: each knob takes its own form and every form built
    on it; SPICEY_NO_READY_ARGS leaves the plan's operand_addr and takes every run-time form; ALL takes everything."""
    fuse, fold, u0, regs, addr = base
    if level == 6:
        return (0, 0, 0, 0, addr)
    if level == 7:
        return (0, 0, 0, 0, 0)
    keep = [level < 1, level < 2, level < 3, level < 4, level < 5]
    return tuple(int(bool(f) and k) for f, k in zip((fuse, fold, u0, regs, addr), keep))


def set_level(monkeypatch, level: int) -> None:
    """The environment of LEVELS[level], and nothing else of the ladder."""
    for k in ALL:
        monkeypatch.delenv(k, raising=False)
    for k in LEVELS[level]:
        monkeypatch.setenv(k, "1")


def chain_circuit():
    """The parsed netlist CHAIN's topology comes from (chain_batch parses the first seed's text)."""
    return parseNetlist(synth.diode_chain(N, seed=1, tran=TRAN))


def spread_diodes(flat):
    """CHAIN's per-instance diode parameters: instance k > 0 has D_is (1 + k) times and D_n = 1 + 0.35 k."""
    for k in range(1, flat.n_inst):
        flat.D_is[k] *= 1 + k
        flat.D_n[k] = 1 + 0.35 * k
    return flat


def chain(n_inst: int, out_nodes=None, replicated: bool = False):
    """CHAIN: diode_chain(511) with `n_inst` instances of their own R, C (seeds 1 ..) and diode parameters; `replicated`: the R
    and C of seed 1 in every instance (the nominal values of a Monte Carlo or sensitivity run).  -> (flat, dt, src[: STEPS + 1])"""
    flat, dt, total, src = synth.chain_batch("diode_chain", N, [1] if replicated else list(range(1, n_inst + 1)), tran=TRAN)
    assert total >= STEPS
    if replicated:
        flat = flat.replicate(n_inst)
    spread_diodes(flat)
    if out_nodes is not None:
        flat.out_nodes = np.ascontiguousarray(out_nodes, dtype=np.int32)
    return flat, dt, src[: STEPS + 1]


def ladder(out_nodes=None):
    """LADDER: the switched ladder of tests/test_packed_resident_gpu.py, 4 instances, several iterations per step."""
    flat, dt, src = _switched_ladder()
    if out_nodes is not None:
        flat.out_nodes = np.ascontiguousarray(out_nodes, dtype=np.int32)
    return flat, dt, src[: STEPS + 1]


def mesh(out_nodes=None):
    """MESH: rcd_mesh(12) twice, the second instance with other R and C."""
    flat, dt, src = _from_text(synth.rcd_mesh(12, tran=TRAN), STEPS)
    flat = flat.replicate(2)
    flat.R_val[1] *= 1.02
    flat.C_val[1] *= 0.99
    if out_nodes is not None:
        flat.out_nodes = np.ascontiguousarray(out_nodes, dtype=np.int32)
    return flat, dt, src


def select_columns(out_v: np.ndarray, out_nodes) -> np.ndarray:
    """What a probe filter must return, from the unfiltered voltages [.., n_nodes]: column node - 1 per entry, +0.0 for ground."""
    nodes = np.asarray(out_nodes)
    picked = out_v[..., np.maximum(nodes, 1) - 1]
    return np.ascontiguousarray(np.where(nodes == 0, 0.0, picked))


def with_state(flat, state):
    """A copy of `flat` that starts from `state` (C_vprev, L_iprev, D_vdprev, S_ison of an earlier run's end)."""
    kw = {k: getattr(flat, k) for k in abi.FlatCircuit.TOPO}
    for k in abi.FlatCircuit.VALS + ("S_ison",):
        kw[k] = np.array(state[k] if k in ("C_vprev", "L_iprev", "D_vdprev", "S_ison") else getattr(flat, k), copy=True)
    kw["out_nodes"] = flat.out_nodes
    return abi.FlatCircuit(flat.n_nodes, flat.n_inst, **kw)


def second_run_sources(ckt, t0: float, dt: float, steps: int) -> np.ndarray:
    """The source rows of a run of `steps` steps of `dt` that starts at time t0: row k is the sources' values at t0 + k dt."""
    tab = np.zeros((steps + 1, len(ckt.V)))
    for j, vs in enumerate(ckt.V):
        tab[:, j] = [vs.waveform(t0 + k * dt) if vs.waveform is not None else (vs.dc or 0.0) for k in range(steps + 1)]
    return tab


def forms_of_plan(flat, steps: int = STEPS):
    """(stamp_fuse_run, top_fold_run, u0_resident_run, top_regs_run, info operand_addr) of spicey_create's plan under the
    current environment, from the three plan harnesses; and the stamp-fuse harness's whole answer."""
    a, t, s = (m.plan(flat, steps=steps, geometry=2) for m in (pyaddr, pytf, pysf))
    assert a["rc"] == t["rc"] == s["rc"] == 0
    assert s["top_fold_run"] == t["top_fold_run"] and a["packed"] == t["packed"] == s["packed"]
    return (s["stamp_fuse_run"], s["top_fold_run"], t["u0_resident_run"], int(bool(t["top_regs"]) and bool(a["addr_run"])), a["info_operand_addr"]), s


@pytest.fixture
def no_knobs(monkeypatch):
    set_level(monkeypatch, 0)
    return monkeypatch


# ---- the plan ---------------------------------------------------------------------------------------------------------------
CIRCUITS = {"chain": lambda: chain(3)[0], "ladder": lambda: ladder()[0], "mesh": lambda: mesh()[0], "bare_node": lambda: chain_with_bare_node(n=N, steps=STEPS)[0]}


@pytest.mark.parametrize("level", range(len(LEVELS)), ids=LEVEL_IDS)
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_every_ladder_level_reports_the_forms_the_gpu_tests_expect(name, level, monkeypatch):
    flat = CIRCUITS[name]()
    set_level(monkeypatch, level)
    forms, s = forms_of_plan(flat)
    assert forms == expected_forms(BASE_FORMS["chain" if name == "bare_node" else name], level), (name, LEVEL_IDS[level], forms)
    assert s["packed"] == 1 and s["threads"] == 512
    assert s["fresh"] == (0 if level == 7 else 1)  # ALL: the default program, the kernel that reads gstat, D_is and dpar where they lie
    if name == "mesh":
        a = pyaddr.plan(flat, steps=STEPS, geometry=2)
        assert (a["early"], a["slots"], a["ready"]) == ((1, 0, 0) if level < 7 else (0, 0, 0))


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_the_plan_folds_and_fuses_under_a_probe_filter_and_diode_parameters(name, no_knobs):
    flat, dt, src = chain(3, FILTERS[name])
    assert not np.array_equal(flat.D_is[0], flat.D_is[1]) and not np.array_equal(flat.D_n[1], flat.D_n[2]) and flat.n_out == len(FILTERS[name])
    forms, s = forms_of_plan(flat)
    assert forms == BASE_FORMS["chain"] and (s["stamp_fuse"], s["top_fold"]) == (1, 1)
    assert forms_of_plan(flat, HALF)[0] == BASE_FORMS["chain"]  # (the step count of the runs with two values of dt)
    # the shards of a MultiHandle over two devices and the 4- and 5-instance handles plan the same kernel
    for n in (2, 4, 5):
        assert forms_of_plan(chain(n)[0])[0] == BASE_FORMS["chain"], n


# ---- the emulator and the oracle --------------------------------------------------------------------------------------------
_FULL: dict = {}


def _unfiltered(fuse: bool):
    """CHAIN with 3 instances, all nodes: the emulator's run, once per form, never modified."""
    if fuse not in _FULL:
        flat, dt, src = chain(3)
        r = pysf.run(flat, STEPS, dt, src, fuse=fuse)
        assert r["status"] == 0 and r["table_ok"] == 1 and r["fold_ok"] == 1
        for a in (r["out_v"], r["out_i"], r["iters"], *r["state"].values()):
            a.setflags(write=False)
        _FULL[fuse] = (flat, dt, src, r)
    return _FULL[fuse]


def _same_bytes(a, b, what, keys=("out_v", "out_i", "iters")):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)
    for k, v in b["state"].items():
        assert np.asarray(a["state"][k]).tobytes() == np.asarray(v).tobytes(), (what, "state", k)
    assert a["solves"] == b["solves"] and a["status"] == b["status"], what


@pytest.mark.parametrize("fuse", [True, False], ids=["fuse", "no_fuse"])
@pytest.mark.parametrize("name", sorted(FILTERS))
def test_a_filtered_run_is_the_column_selection_of_the_unfiltered_run(name, fuse, no_knobs):
    nodes = FILTERS[name]
    _, dt, src, full = _unfiltered(fuse)
    flat, _, _ = chain(3, nodes)
    for currents in (True, False):
        got = pysf.run(flat, STEPS, dt, src, fuse=fuse, currents=currents, nan_fill=True)
        assert got["status"] == 0 and got["out_v"].shape == (3, STEPS + 1, len(nodes))
        assert got["out_v"].tobytes() == select_columns(full["out_v"], nodes).tobytes(), (name, currents)
        if 0 in nodes:
            col = got["out_v"][:, :, nodes.index(0)]
            assert not col.any() and not np.signbit(col).any()
        _same_bytes(got, full, (name, currents), keys=("out_i", "iters") if currents else ("iters",))


def meets_oracle(got, j, ref, what, label="forms-ratio", currents=True):
    """Instance j of a result against the one-instance oracle result `ref` at the bar, end state (D_vdprev too) included.
    Prints the share of the bar it used; returns the largest share."""
    rv = float(tol_ratio(got["out_v"][j], ref["out_v"][0]).max())
    ri = float(tol_ratio(got["out_i"][j], ref["out_i"][0]).max()) if currents else 0.0
    rs = max(float(tol_ratio(got["state"][k][j], ref["state"][k][0]).max()) for k in ("C_vprev", "L_iprev", "D_vdprev"))
    print(f"{label} {what} inst {j}: out_v {rv:.3g} out_i {ri:.3g} state {rs:.3g}")
    assert np.array_equal(got["iters"][j], ref["iters"][0]), what
    assert rv <= 1.0 and ri <= 1.0 and rs <= 1.0, (what, rv, ri, rs)
    assert np.array_equal(got["state"]["S_ison"][j], ref["state"]["S_ison"][0]), what
    return max(rv, ri, rs)


def test_per_instance_diode_parameters_agree_between_the_forms_and_meet_the_oracle(oracle_backend, no_knobs):
    flat, dt, src, fused = _unfiltered(True)
    _, _, _, plain = _unfiltered(False)
    _same_bytes(fused, plain, "diode parameters")
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(fused["out_v"][a], fused["out_v"][b]) and not np.array_equal(fused["state"]["D_vdprev"][a], fused["state"]["D_vdprev"][b])
    for j in range(3):
        ref = oracle_backend.run(instance(flat, j), STEPS, dt, src)
        assert ref["status"] == 0
        meets_oracle(fused, j, ref, "emulator, diode parameters")
    # the diode parameters, not only R and C, tell the instances apart: the R and C of seed 1 everywhere
    same_rc, _, _ = chain(3, replicated=True)
    r = pysf.run(same_rc, STEPS, dt, src, fuse=True)
    assert r["status"] == 0 and not np.array_equal(r["out_v"][0], r["out_v"][1]) and not np.array_equal(r["out_v"][1], r["out_v"][2])
    ref = oracle_backend.run(instance(same_rc, 2), STEPS, dt, src)
    meets_oracle(r, 2, ref, "emulator, diode parameters alone")


def test_a_second_run_with_half_the_step_agrees_between_the_forms_and_meets_the_oracle(oracle_backend, no_knobs):
    flat, dt, src = chain(3)
    src2 = second_run_sources(chain_circuit(), HALF * dt, dt / 2, HALF)
    assert np.array_equal(src2[0], src[HALF])
    runs = {}
    for fuse in (True, False):
        r1 = pysf.run(flat, HALF, dt, src[: HALF + 1], fuse=fuse)
        r2 = pysf.run(flat, HALF, dt / 2, src2, fuse=fuse, state=r1["state"], nan_fill=True)
        same_dt = pysf.run(flat, HALF, dt, src2, fuse=fuse, state=r1["state"])
        assert r1["status"] == r2["status"] == same_dt["status"] == 0
        runs[fuse] = (r1, r2, same_dt)
    for k, what in enumerate(("run 1", "run 2 at dt / 2", "run 2 at dt")):
        _same_bytes(runs[True][k], runs[False][k], what)
    r1, r2, same_dt = runs[True]
    assert not np.array_equal(r2["out_v"], same_dt["out_v"]) and not np.array_equal(r2["out_v"], r1["out_v"])
    _, _, _, full = _unfiltered(True)
    assert r1["out_v"].tobytes() == np.ascontiguousarray(full["out_v"][:, : HALF + 1]).tobytes()
    for j in range(3):
        ref = oracle_backend.run(instance(with_state(flat, r1["state"]), j), HALF, dt / 2, src2)
        assert ref["status"] == 0
        meets_oracle(r2, j, ref, "emulator, second run at dt / 2")


def test_the_when_threshold_is_crossed_well_inside_the_run(oracle_backend, no_knobs):
    """The threshold the GPU module's when("v(n64)", WHEN_LEVEL) uses, on the oracle's waveforms of the four CHAIN instances and of
    the replicated chain a Monte Carlo run starts from: one rising crossing, at least 8 steps from either end."""
    for replicated in (False, True):
        flat, dt, src = chain(4, replicated=replicated)
        for j in range(4):
            v = oracle_backend.run(instance(flat, j), STEPS, dt, src)["out_v"][0][:, 63]
            up = np.nonzero((v[:-1] < WHEN_LEVEL) & (v[1:] >= WHEN_LEVEL))[0]
            assert len(up) == 1 and 8 <= up[0] and up[0] + 1 <= STEPS - 8, (replicated, j, up)
            assert abs(v[up[0]] - WHEN_LEVEL) > 1e-6 and abs(v[up[0] + 1] - WHEN_LEVEL) > 1e-6  # (no sample sits on the threshold)


def test_the_chain_with_a_bare_node_fuses_at_511_and_fails_the_same_way_in_both_forms(no_knobs):
    """n = 511 with D2 and C2 cut still takes the fuse (the GPU module's singular Monte Carlo sample runs on it): instance 1 of
    three has a pivot of 2e-16 in the matrix of step 0, and both forms name that instance, step and iteration."""
    flat, dt, src = chain_with_bare_node(n=N, steps=STEPS)
    assert forms_of_plan(flat)[0] == BASE_FORMS["chain"]
    per = np.ascontiguousarray(np.broadcast_to(src, (3, STEPS + 1, flat.nV)))
    got, ref = (pysf.run(flat, STEPS, dt, per, fuse=f) for f in (True, False))
    assert got["status"] == ref["status"] == abi.ERR_SINGULAR and got["err4"].tolist() == ref["err4"].tolist() == [1, 1, 0, 0]
    for j in (0, 2):
        assert got["out_v"][j].tobytes() == ref["out_v"][j].tobytes() and got["iters"][j].all()
