"""Fresh-fill programs (spicey_build_program's fresh_fill, program.h: nKeep) on the CPU: the builder's invariants on the program
as the device gets it, emulator runs of the packed layout (512 threads, 4 slots) on the fresh build against the default
program on the default build — same bits, also from a workspace that starts as NaN — and the launch plan's choice.

The harness is tests/fresh_host (it compiles the emulator's sources unchanged)."""
from __future__ import annotations

import numpy as np
import pytest

from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist

from conftest import SMALL_GOLDENS, golden_netlist, load_golden
from fresh_host import pyfresh
from test_packed_resident_gpu import _switched_ladder

STEPS = 64


def _flat(text):
    return abi.flatten(parseNetlist(text), probe_filter=True)


def _switched_text():
    flat, _, _ = _switched_ladder()
    return flat


BUILDER_CASES = {f"diode_chain({n})": (lambda n=n: _flat(synth.diode_chain(n))) for n in (20, 100, 333, 1000, 1023)}
BUILDER_CASES.update({f"rc_ladder({n})": (lambda n=n: _flat(synth.rc_ladder(n))) for n in (20, 1000)})
BUILDER_CASES.update({f"rcd_mesh({r})": (lambda r=r: _flat(synth.rcd_mesh(r))) for r in (6, 12, 15)})
BUILDER_CASES["switched_ladder"] = _switched_text
BUILDER_CASES.update({f"golden:{g}": (lambda g=g: _flat(golden_netlist(load_golden(g)))) for g in SMALL_GOLDENS})

VIOLATIONS = ("stamped_in_class", "not_one_flag", "flag_not_in_first_phase", "read_before_created", "flag_outside_class", "encodings_differ",
              "untargeted_but_touched")


@pytest.mark.parametrize("top", [True, False], ids=["top", "no_top"])
@pytest.mark.parametrize("case", sorted(BUILDER_CASES))
def test_builder_invariants(case, top):
    flat = BUILDER_CASES[case]()
    got = pyfresh.check(flat, pcr_top=top, fresh=True)
    assert got["rc"] == 0
    assert 0 <= got["nKeep"] <= got["nRestore"] <= got["nLU"]
    for k in VIOLATIONS:
        assert got[k] == 0, (case, k, got)
    # without the option the class is empty and no record carries a flag
    off = pyfresh.check(flat, pcr_top=top, fresh=False)
    assert off["rc"] == 0 and off["nKeep"] == off["nRestore"] == got["nRestore"] and off["flag_outside_class"] == 0
    if case in ("diode_chain(1000)", "rc_ladder(1000)", "switched_ladder", "rcd_mesh(12)"):
        assert got["has16"] == 1 and got["fresh_entries"] > 0  # (the checks above are not vacuous)


def test_the_bench_chain_keeps_about_a_thousand_entries():
    got = pyfresh.check(_flat(synth.diode_chain(1000)))
    # ~2 000 of the ~3 000 re-stamped entries are pure fill: 1 000 diagonals and the source's row stay
    assert got["nKeep"] == 1001 and got["nRestore"] == 2966 and got["fresh_entries"] >= 1800


def _chain(kind, n):
    flat, dt, steps, src = synth.chain_batch(kind, n, [3], tran=".tran 1e-6 7e-5")
    assert steps >= STEPS
    return flat, dt, src[: STEPS + 1]


def _mesh12():
    ckt = parseNetlist(synth.rcd_mesh(12, tran=".tran 1e-6 7e-5"))
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    assert steps >= STEPS
    return abi.flatten(ckt), dt, abi.source_table(ckt, dt, steps)[: STEPS + 1]


def _mesh15():
    ckt = parseNetlist(synth.rcd_mesh(15, tran=".tran 1e-6 3.2e-5"))
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    return abi.flatten(ckt), dt, abi.source_table(ckt, dt, steps)


def _golden(name):
    """A small golden over its own .tran (the run's length is the table's)."""
    ckt = parseNetlist(golden_netlist(load_golden(name)))
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    return abi.flatten(ckt), dt, abi.source_table(ckt, dt, steps)


def _switched_one():
    flat, dt, src = _switched_ladder()
    from batch_variants import instance
    return instance(flat, 2), dt, src


RUN_CASES = {
    "diode_chain_1000": lambda: _chain("diode_chain", 1000),  # every lane of the streamed level has a row record
    "diode_chain_600": lambda: _chain("diode_chain", 600),    # fewer row records than threads
    "rc_ladder_1000": lambda: _chain("rc_ladder", 1000),      # factor reuse: the fills of step 0 are kept
    "switched_ladder": _switched_one,                         # iterations > 1
    "rcd_mesh_12": _mesh12,                                   # overflow lists, entries targeted at several levels
    # the CPU twins of tests/test_packed_topologies_gpu.py: when a case fails there, these say whether the program is wrong
    "diode_chain_1023": lambda: _chain("diode_chain", 1023),  # nKeep == 2 x 512, more than one streamed phase
    "diode_chain_511": lambda: _chain("diode_chain", 511),    # n around the workgroup size
    "diode_chain_513": lambda: _chain("diode_chain", 513),
    "rcd_mesh_15": _mesh15,                                   # nRestore just under 6 x 512
}
# small goldens with a fresh class: switches, inductors, diodes, everything in the LDS tail levels
TAIL_GOLDENS = ("boost_probe", "half_bridge", "diode_switch", "switch_vt_vh", "vswitch_pwl", "relay_osc", "star_hub", "bridge_bleed", "dchain20", "mesh9x5")
RUN_CASES.update({f"golden:{g}": (lambda g=g: _golden(g)) for g in TAIL_GOLDENS})
_DEFAULT: dict = {}


def _default_run(case):
    """The default program on the default packed build: computed once per case, never modified."""
    if case not in _DEFAULT:
        flat, dt, src = RUN_CASES[case]()
        r = pyfresh.run(flat, len(src) - 1, dt, src, fresh=False)
        assert r["status"] == 0 and r["fresh_fill"] == 0 and r["nKeep"] == r["nRestore"]
        for a in (r["out_v"], r["out_i"], r["iters"], *r["state"].values()):
            a.setflags(write=False)
        _DEFAULT[case] = (flat, dt, src, r)
    return _DEFAULT[case]


@pytest.mark.parametrize("nan_fill", [False, True], ids=["zeroed", "nan_arena"])
@pytest.mark.parametrize("case", sorted(RUN_CASES))
def test_fresh_program_gives_the_default_programs_bits(case, nan_fill):
    flat, dt, src, ref = _default_run(case)
    got = pyfresh.run(flat, len(src) - 1, dt, src, fresh=True, nan_fill=nan_fill)
    assert got["status"] == 0 and got["fresh_fill"] == 1
    assert got["nRestore"] == ref["nRestore"] and got["nKeep"] < got["nRestore"]
    assert (got["streamed_tasks"], got["resident_tasks"]) == (ref["streamed_tasks"], ref["resident_tasks"])
    assert np.isfinite(got["out_v"]).all() and np.isfinite(got["out_i"]).all()
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(got[k], ref[k]), (case, k)
    for k, v in ref["state"].items():
        assert np.array_equal(got["state"][k], v), (case, k)
    if case == "switched_ladder":
        assert int(got["iters"].max()) > 1
    if case == "diode_chain_1000":
        assert got["streamed_tasks"] == 2000 and got["resident_tasks"] == 2719
    if case == "diode_chain_1023":
        assert got["nKeep"] == 2 * 512 and got["streamed_tasks"] == 3070
    if case == "rcd_mesh_15":
        assert (got["nKeep"], got["nRestore"], got["streamed_tasks"]) == (266, 2930, 17188)
    if case in ("golden:half_bridge", "golden:diode_switch", "golden:switch_vt_vh", "golden:vswitch_pwl", "golden:relay_osc"):
        assert int(got["iters"].max()) > 1  # (a switch flips within the golden's own .tran)


RANDOM_BLOCK = 40


@pytest.mark.parametrize("nan_fill", [False, True], ids=["zeroed", "nan_arena"])
@pytest.mark.parametrize("floating,first", [(False, s) for s in range(0, 200, RANDOM_BLOCK)] + [(True, s) for s in range(0, 120, RANDOM_BLOCK)],
                         ids=lambda v: {False: "grounded", True: "floating"}[v] if isinstance(v, bool) else f"seeds_{v}")
def test_fresh_program_gives_the_default_programs_bits_on_random_circuits(floating, first, nan_fill):
    """tests/random_circuits.py, seeds 0..199 and 0..119 with floating sources (every one packable): R / C / L / V / D / S
    mixes of a few unknowns, everything in the LDS tail levels."""
    from random_circuits import random_netlist
    with_class = 0
    for seed in range(first, first + RANDOM_BLOCK):
        ckt = parseNetlist(random_netlist(seed, floating_sources=floating))
        dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
        flat, src = abi.flatten(ckt), abi.source_table(ckt, dt, steps)
        ref = pyfresh.run(flat, steps, dt, src, fresh=False)
        got = pyfresh.run(flat, steps, dt, src, fresh=True, nan_fill=nan_fill)
        assert ref["status"] == got["status"] == 0 and ref["fresh_fill"] == 0 and got["fresh_fill"] == 1, seed
        assert ref["nKeep"] == ref["nRestore"] == got["nRestore"] and got["nKeep"] <= got["nRestore"], seed
        with_class += int(got["nKeep"] < got["nRestore"])
        assert np.isfinite(got["out_v"]).all(), seed
        for k in ("out_v", "out_i", "iters"):
            assert np.array_equal(got[k], ref[k], equal_nan=(k == "out_i")), (seed, k)
        for k, v in ref["state"].items():
            assert np.array_equal(got["state"][k], v), (seed, k)
    assert with_class >= RANDOM_BLOCK - 1  # (one seed of the 200 has no fill to create)


def test_threads_in_reverse_order_change_nothing():
    flat, dt, src, ref = _default_run("diode_chain_600")
    got = pyfresh.run(flat, len(src) - 1, dt, src, fresh=True, nan_fill=True, reverse=True)
    assert got["status"] == 0
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(got[k], ref[k])


# ---- the launch plan ------------------------------------------------------------------------------------------------------
def _bench_batch(n=1000, n_inst=512):
    return _flat(synth.diode_chain(n)).replicate(n_inst)


def test_the_bench_batch_takes_the_fresh_build(monkeypatch):
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL", raising=False)
    monkeypatch.delenv("SPICEY_FRESH_FILL_LINEAR", raising=False)
    p = pyfresh.plan(_bench_batch())
    assert p["rc"] == 0 and p["packed"] == 1 and p["fresh"] == 1 and p["program_fresh_fill"] == 1 and p["threads"] == 512
    assert p["nKeep"] <= 2 * 512 and p["nDynEnt"] <= 2 * 512 and p["nKeep"] < p["nRestore"]
    assert p["shape"] == 1  # (SPICEY_V2_SHAPES: the <4, 2, 2> build)
    info = p["info"]
    assert info["geometry"] == 2 and info["resident_slots"] == 4 and info["streamed_tasks"] == 2000 and info["resident_tasks"] == 2719


def test_the_switch_keeps_the_default_program(monkeypatch):
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL", raising=False)
    on = pyfresh.plan(_bench_batch())
    monkeypatch.setenv("SPICEY_NO_FRESH_FILL", "1")
    off = pyfresh.plan(_bench_batch())
    assert off["rc"] == 0 and off["packed"] == 1 and off["fresh"] == 0 and off["program_fresh_fill"] == 0 and off["shape"] == 0
    assert off["nKeep"] == off["nRestore"] == on["nRestore"]
    for k in ("geometry", "threads", "resident_slots", "streamed_tasks", "resident_tasks", "lds_bytes", "tail_levels", "pcr_rows", "pcr_level"):
        assert off["info"][k] == on["info"][k], k


def _series_diode_ladder(n):
    L = ["* series diodes", ".model DM D(Is=1e-14 N=1)", "V1 n1 0 PULSE(0 5 0 1e-6 1e-6 4e-6 1e-5)"]
    for k in range(1, n):
        L += [f"D{k} n{k} n{k+1} DM", f"R{k} n{k} n{k+1} 1k", f"C{k} n{k+1} 0 1n"]
    return "\n".join(L + [".tran 1e-6 7e-5", ".end", ""])


def test_a_circuit_with_too_many_kept_entries_keeps_the_default_build(monkeypatch):
    """A circuit the packed geometry takes whose kept entries exceed 2 x 512.  No R/C/diode mesh of up to 1 024 unknowns is
    one: over every rcd_mesh(rows, cols) with rows <= 32 that the packed geometry accepts, the largest nKeep is 332
    (3 x 133; a mesh's fill outweighs its kept entries, and nRestore <= 6 x 512 bounds the geometry first).  A ladder of
    400 nodes with a diode in every series branch is: three dynamic entries per node, 1 199 kept."""
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL", raising=False)
    flat = _flat(_series_diode_ladder(400))
    chk = pyfresh.check(flat)
    assert chk["nKeep"] > 2 * 512 and chk["fresh_entries"] > 0
    p = pyfresh.plan(flat.replicate(4), geometry=2)
    assert p["rc"] == 0 and p["packed"] == 1
    assert p["fresh"] == 0 and p["program_fresh_fill"] == 0 and p["shape"] == 0 and p["nKeep"] == p["nRestore"]
    # ... and a mesh, with few kept entries, takes the fresh build
    m = pyfresh.plan(_flat(synth.rcd_mesh(12)).replicate(4), geometry=2)
    assert m["rc"] == 0 and m["packed"] == 1 and m["fresh"] == 1 and m["nKeep"] <= 2 * 512


def test_a_linear_circuit_keeps_the_default_program(monkeypatch):
    """Factor reuse: B re-stamps nothing after step 0, so the fresh class has nothing to save there."""
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL", raising=False)
    monkeypatch.delenv("SPICEY_FRESH_FILL_LINEAR", raising=False)
    flat = _flat(synth.rc_ladder(1000)).replicate(512)
    p = pyfresh.plan(flat)
    assert p["rc"] == 0 and p["packed"] == 1 and p["fresh"] == 0 and p["program_fresh_fill"] == 0 and p["shape"] == 0
    monkeypatch.setenv("SPICEY_FRESH_FILL_LINEAR", "1")  # (tests: the fresh build on a reused factorisation)
    q = pyfresh.plan(flat)
    assert q["fresh"] == 1 and q["shape"] == 1 and q["info"]["streamed_tasks"] == p["info"]["streamed_tasks"]


def test_the_latency_geometry_keeps_the_default_program(monkeypatch):
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL", raising=False)
    p = pyfresh.plan(_flat(synth.diode_chain(1000)).replicate(4), geometry=1)
    assert p["rc"] == 0 and p["packed"] == 0 and p["fresh"] == 0 and p["program_fresh_fill"] == 0
