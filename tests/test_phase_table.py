"""The phase table of the 16-bit interpreter (spicey_amd/csrc/tran_exec.h): the run-invariant arguments of the time loop's
phases — record bases and counts of the streamed phases, element counts, per-run pointers — are written once into the tail
area behind the tridiagonal top's index table and read from there by every phase; programs without room for it, and runs
with SPICEY_NO_PHASE_TABLE set, fetch them from the argument structs in every phase as before.

The change moves where addresses and counts come from, not one floating-point operation: both paths must give identical
bits.  The emulator runs the same table-building and table-reading code as the kernels (one word per "lane" on the GPU, a
plain index here) and decides per run, from the environment, which path to take."""
import os
import random

import numpy as np
import pytest

from conftest import golden_netlist, load_golden
from emul.pyemul import EmulBackend
from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist

KNOB = "SPICEY_NO_PHASE_TABLE"


def _golden(name, steps=None):
    ckt = parseNetlist(golden_netlist(load_golden(name)))
    return _circuit(ckt, steps)


def _circuit(ckt, steps=None):
    tr = ckt.analyses["tran"]
    dt, n = abi.computeEffectiveTimeStep(tr["dt"], tr["tstop"])
    if steps is not None and steps < n:
        n = steps
    return abi.flatten(ckt), n, dt, abi.source_table(ckt, dt, n)[: n + 1]


def table_fits(info):
    """spicey_pt_fits of tran_exec.h: a tridiagonal top (which excludes tail levels), and the run-wide block (48 words) plus
    one 8-word row per streamable phase (2 x pcr_level) behind the top's row buffers (1024 words) and index table
    (2 x pcr_rows words, rounded up to 4) inside the 5 KB (1280 words) tail area."""
    n, lvl = info["pcr_rows"], info["pcr_level"]
    return 0 < n <= 64 and lvl >= 1 and 1024 + ((2 * n + 3) & ~3) + 48 + 16 * lvl <= 1280


def both_paths(flat, steps, dt, src, **kw):
    """One run with the table (where the program has room for it) and one without; returns (with, without, info)."""
    assert KNOB not in os.environ
    be = EmulBackend(**kw)
    on = be.run(flat, steps, dt, src)
    info = be.info
    os.environ[KNOB] = "1"
    try:
        off = EmulBackend(**kw).run(flat, steps, dt, src)
    finally:
        del os.environ[KNOB]
    return on, off, info


def assert_same_bits(a, b, what):
    assert a["status"] == 0 and b["status"] == 0, (what, a["detail"], b["detail"])
    for k in ("out_v", "out_i"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64)), (what, k)
    assert np.array_equal(a["iters"], b["iters"]), (what, "iters")
    for k in a["state"]:
        x, y = np.ascontiguousarray(a["state"][k]), np.ascontiguousarray(b["state"][k])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, "state", k)


# (threads, reversed thread order inside every phase, resident slots): few slots and threads — most phases streamed, the
# beyond-resident loops of B and Z at work (they read the argument structs, not the table) — and many
SHAPES = [(64, False, 2), (128, True, 8), (512, False, 16)]


def test_dchain1000_200_table_and_scalar_loads_identical(oracle_backend):
    """The headline circuit (1000-node diode chain): tridiagonal top at level 4 on 512 threads, the wide factor levels
    streamed from row records."""
    flat, steps, dt, src = _golden("dchain1000_200", steps=24)
    ref = oracle_backend.run(flat, steps, dt, src)
    for T, rev, rmax in SHAPES + [(512, False, 4)]:
        on, off, info = both_paths(flat, steps, dt, src, K=1, T=T, reverse=rev, rmax=rmax)
        assert info["pcr_rows"] > 0 and table_fits(info), info
        assert_same_bits(on, off, ("dchain1000_200", T, rev, rmax))
        err = np.abs(on["out_v"] - ref["out_v"]) / (1e-9 * np.abs(ref["out_v"]) + 1e-12)
        assert err.max() <= 1.0
    # without the row records the streamed factor phases take the generic 16-byte records: the other half of a table row
    on, off, info = both_paths(flat, steps, dt, src, K=1, T=128, rmax=2, no_rows=True)
    assert table_fits(info)
    assert_same_bits(on, off, "dchain1000_200 without row records")


def switched_ladder(n, seed):
    """A long ladder with series switches (driven by a second source) and shunt diodes: switch iterations on a circuit
    that has a tridiagonal top and row records."""
    rng = random.Random(seed)
    L = ["* switched ladder", ".model SW SW(Ron=1 Roff=1e6 Vt=2.5 Vh=0.2)", ".model DM D(Is=1e-14 N=1)",
         "V1 n1 0 PULSE(0 5 0 1e-6 1e-6 4e-6 1e-5)", "VC ctl 0 PULSE(0 5 2e-6 1e-6 1e-6 3e-6 8e-6)"]
    for k in range(1, n):
        if k % 37 == 0:
            L.append(f"S{k} n{k} n{k+1} ctl 0 SW")
        else:
            L.append(f"R{k} n{k} n{k+1} {100 * (1 + 0.1 * rng.random()):.6g}")
        L.append(f"C{k} n{k+1} 0 {1e-9 * (1 + 0.1 * rng.random()):.6g}")
        if rng.random() < 0.5:
            L.append(f"D{k} n{k+1} 0 DM")
    L += [".tran 1e-6 1.2e-5", ".end", ""]
    return "\n".join(L)


def test_switches_iteration_loop_identical(oracle_backend):
    """Switches: the iteration loop with phases S and A between the solves, B and Z with their switch loops (which read the
    argument structs inside their own branch while the rest of the phase runs from the table)."""
    for n in (200, 520):
        flat, steps, dt, src = _circuit(parseNetlist(switched_ladder(n, seed=n)))
        assert flat.nS > 0
        ref = oracle_backend.run(flat, steps, dt, src)
        for T, rev, rmax in SHAPES:
            on, off, info = both_paths(flat, steps, dt, src, K=1, T=T, reverse=rev, rmax=rmax)
            assert table_fits(info), info
            assert_same_bits(on, off, ("switched ladder", n, T, rev, rmax))
            assert on["iters"].max() >= 2  # (the iteration loop ran)
            assert np.array_equal(on["iters"], ref["iters"]) and np.array_equal(on["state"]["S_ison"], ref["state"]["S_ison"])
    # small switched goldens (no top: the scalar loads either way)
    for name in ("half_bridge", "boost_probe"):
        flat, steps, dt, src = _golden(name, steps=300)
        on, off, info = both_paths(flat, steps, dt, src, K=1, T=64, rmax=8)
        assert_same_bits(on, off, name)


def test_linear_circuit_factor_reuse_identical():
    """A linear ladder keeps the factors of step 0: later steps run the right-hand-side column only, whose record counts
    are the `rhs` fields of a table row, and the row targets below xoff are skipped (xoff comes from the table too)."""
    ckt = parseNetlist(synth.rc_ladder(600, seed=7, tran=".tran 1e-6 3e-5"))
    flat, steps, dt, src = _circuit(ckt)
    for T, rev, rmax in SHAPES:
        on, off, info = both_paths(flat, steps, dt, src, K=1, T=T, reverse=rev, rmax=rmax)
        assert table_fits(info), info
        assert_same_bits(on, off, ("rc_ladder", T, rev, rmax))
        # and the reuse path against refactoring every step
        refac, _, _ = both_paths(flat, steps, dt, src, K=1, T=T, reverse=rev, rmax=rmax, no_reuse=True)
        assert_same_bits(on, refac, ("rc_ladder reuse vs refactor", T, rev, rmax))


def test_hybrid_layout_chain_identical():
    """Hybrid workspace: the two phases of the leaves read their operands from the global array and need xoff at their
    head; B and Z keep the scalar loads in these builds, the factor / backward phases take the table."""
    ckt = parseNetlist(synth.diode_chain(300, seed=4, tran=".tran 1e-6 1.5e-5"))
    flat, steps, dt, src = _circuit(ckt)
    plain = EmulBackend(1, 128, False, 8).run(flat, steps, dt, src)
    for rmax in (6, 8, 16):
        on, off, info = both_paths(flat, steps, dt, src, K=1, T=128, rmax=rmax, hybrid=True)
        assert info["hybrid_entries"] > 0 and table_fits(info), info
        assert_same_bits(on, off, ("hybrid diode_chain(300)", rmax))
        assert_same_bits(on, plain, ("hybrid against the all-LDS layout", rmax))


def test_without_a_top_the_scalar_loads_stay():
    """No tridiagonal top: the tail area is as large as the tail levels need and holds their records — no room for the
    table, the run takes the scalar loads whatever the knob says.  A mesh has no top by construction; a chain is run with
    the top switched off."""
    for name, kw in (("mesh20_30", dict()), ("dchain1000_200", dict(no_pcr=True)), ("mesh9x5", dict())):
        flat, steps, dt, src = _golden(name, steps=20)
        for T, rev, rmax in SHAPES[:2]:
            on, off, info = both_paths(flat, steps, dt, src, K=1, T=T, reverse=rev, rmax=rmax, **kw)
            assert info["pcr_rows"] == 0 and not table_fits(info)
            assert_same_bits(on, off, (name, T, rev, rmax))


@pytest.mark.parametrize("n", [2000, 4000])
def test_deep_tree_rows_beyond_the_tail_area_fall_back(n):
    """A longer chain has its top at a higher level: from pcr_level 6 on the rows no longer fit behind a 64-row index
    table (1152 + 48 + 16 x 6 > 1280 words) and the run must not write past the tail area.  Either way: same bits."""
    ckt = parseNetlist(synth.diode_chain(n, seed=2, tran=".tran 1e-6 6e-6"))
    flat, steps, dt, src = _circuit(ckt)
    on, off, info = both_paths(flat, steps, dt, src, K=1, T=512, rmax=8)
    assert info["pcr_rows"] > 0
    assert_same_bits(on, off, ("diode_chain", n, "fits" if table_fits(info) else "falls back"))


def test_diagnostics_read_their_arguments_inside_their_branch():
    """SpiceyOptions.diagnostics bit 1 (per-step linearisation error): Z's diagnostics pass reads the diode terminals from
    the argument structs inside its own branch, its pointers from the table."""
    flat, steps, dt, src = _golden("dchain1000_200", steps=12)
    on, off, info = both_paths(flat, steps, dt, src, K=1, T=128, rmax=8, diagnostics=3)
    assert table_fits(info)
    assert_same_bits(on, off, "diagnostics")
    assert np.array_equal(on["lin_err"], off["lin_err"]) and np.array_equal(on["skip_risk"], off["skip_risk"])
    assert on["lin_err"].max() > 0.0
