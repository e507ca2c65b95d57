"""The reference-order engine (SpiceyOptions.interpreter = 3) on the CPU: the product's plan (launch_plan.cpp), stamp
lists (exact_plan.cpp) and phase code (exact_exec.h) run by tests/exact_host/harness.cpp with a serial executor, at 64 and
256 threads, in the LDS and the global layout, checked bit for bit against the reference-generated goldens and the oracle
(oracle/spicey_ref.c)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import (PROBE_GOLDENS, QUIRK_GOLDENS, SINGULAR_GOLDENS, SKIP_CASES, SMALL_GOLDENS, bits_equal, farr, golden_netlist,
                      load_golden)
from spicey_amd import abi
from spicey_amd.netlist import parseNetlist
from spicey_amd.simulate import SingularMatrixError, formatTranResult, simulateTRAN

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "exact_host"))
from pyexact import ExactHostBackend, stamp_lists  # noqa: E402

LAYOUTS = [dict(T=64), dict(T=256), dict(T=64, global_ws=True), dict(T=256, global_ws=True, reverse=True)]


def _setup(text):
    ckt = parseNetlist(text)
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    return abi.flatten(ckt), steps, dt, abi.source_table(ckt, dt, steps)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["T64", "T256", "T64_global", "T256_global_reverse"])
@pytest.mark.parametrize("name", SMALL_GOLDENS + QUIRK_GOLDENS + sorted(SKIP_CASES) + PROBE_GOLDENS)
def test_goldens_bit_exact(name, layout):
    g = load_golden(name)
    ckt = parseNetlist(golden_netlist(g))
    for ri, run in enumerate(g["runs"]):  # run 2 continues from run 1's end state
        res = simulateTRAN(ckt, backend=ExactHostBackend(**layout))
        assert list(res["nodeVoltages"]) == run["keysV"] and list(res["elementCurrents"]) == run["keysI"]
        assert res["times"] == run["times"]
        for k in run["keysV"]:
            assert bits_equal(res["nodeVoltages"][k], farr(run["V"][k])).all(), (name, ri, k)
        for k in run["keysI"]:
            assert bits_equal(res["elementCurrents"][k], farr(run["I"][k])).all(), (name, ri, k)
        assert [c.vPrev for c in ckt.C] == run["state"]["C_vPrev"] and [l.iPrev for l in ckt.L] == run["state"]["L_iPrev"]
        assert [d.vdPrev for d in ckt.D] == run["state"]["D_vdPrev"] and [int(s.isOn) for s in ckt.S] == run["state"]["S_isOn"]
        if ri == 0 and "formatted_head" in run:
            assert formatTranResult(res).split("\n")[:4] == run["formatted_head"]


@pytest.mark.parametrize("name", SINGULAR_GOLDENS)
def test_singular_goldens(name):
    for layout in LAYOUTS:
        with pytest.raises(SingularMatrixError):
            simulateTRAN(parseNetlist(golden_netlist(load_golden(name))), backend=ExactHostBackend(**layout))


@pytest.mark.parametrize("name", sorted(SKIP_CASES))
def test_skip_count_is_the_oracles(name, oracle_backend):
    """diagnostics bit 0 in exact mode = the nonzero multipliers the reference's |f| < EPS test dropped (skip_clamp_floor
    included, which the default path's indicator misses)."""
    flat, steps, dt, src = _setup(golden_netlist(load_golden(name)))
    got = ExactHostBackend().run(flat, steps, dt, src)
    ref = oracle_backend.run(flat, steps, dt, src)
    assert np.array_equal(got["skip_risk"], ref["skipped"]) and (ref["skipped"][0] > 0) == SKIP_CASES[name][0]
    assert bits_equal(got["lin_err"], ref["lin_err"]).all()


def _same(got, ref, seed):
    assert got["status"] == ref["status"], (seed, got["detail"], ref["detail"])
    if ref["status"] != 0:
        assert got["detail"] == ref["detail"], seed
        return
    assert np.array_equal(got["iters"], ref["iters"]), seed
    assert bits_equal(got["out_v"], ref["out_v"]).all() and bits_equal(got["out_i"], ref["out_i"]).all(), seed
    for k in ("C_vprev", "L_iprev", "D_vdprev"):
        assert bits_equal(got["state"][k], ref["state"][k]).all(), (seed, k)
    assert np.array_equal(got["state"]["S_ison"], ref["state"]["S_ison"]), seed
    assert np.array_equal(got["skip_risk"], ref["skipped"]) and bits_equal(got["lin_err"], ref["lin_err"]).all(), seed


RANDOM_SEEDS = [(s, {}) for s in range(200)] + [(693, dict(floating_sources=True))] + [(s, dict(max_nodes=14)) for s in (467, 2011, 2610, 2833, 2703)]


def test_random_circuits_bit_identical_to_the_oracle(oracle_backend):
    """Seeds 0..199 (the nine the GPU parity loop leaves out included) and the soak outliers: the oracle's status, and its
    bits wherever it is OK."""
    from random_circuits import random_netlist
    ok = 0
    for i, (seed, kw) in enumerate(RANDOM_SEEDS):
        flat, steps, dt, src = _setup(random_netlist(seed, **kw))
        ref = oracle_backend.run(flat, steps, dt, src)
        got = ExactHostBackend(**LAYOUTS[i % len(LAYOUTS)]).run(flat, steps, dt, src)
        _same(got, ref, seed)
        ok += ref["status"] == 0
    assert ok > 150


def test_batch_of_distinct_instances(oracle_backend):
    from spicey_amd import synth
    flats = [_setup(synth.diode_chain(12, seed=s, tran=".tran 1e-6 1e-5")) for s in range(5)]
    flat = abi.stack_instances([f[0] for f in flats])
    steps, dt, src = flats[0][1:]
    for layout in LAYOUTS:
        _same(ExactHostBackend(**layout).run(flat, steps, dt, src), oracle_backend.run(flat, steps, dt, src), layout)


def test_stamp_lists_in_the_reference_order():
    """Parallel duplicates on one node pair, every element kind, a floating source, an element with both ends on ground."""
    text = """* stamp order
R1 1 2 1k
R2 1 2 2k
C1 2 0 1u
L1 2 3 1m
R3 0 0 5
S1 3 0 1 0 SW
.model SW VSWITCH(Ron=1 Roff=1e6 Von=1 Voff=0.5)
V1 1 0 DC 5
V2 3 2 DC 1
D1 2 1 DM
.model DM D(Is=1e-14 N=1)
.tran 1e-6 1e-5
.end
"""
    ckt = parseNetlist(text)
    flat = abi.flatten(ckt)
    lists = dict(stamp_lists(flat))
    n = flat.n_var  # 3 nodes + 2 sources
    assert n == 5
    # a_11: R1, R2, then V1's +1 is not on the diagonal; D1 (anode 2, cathode 1) adds gd last
    assert lists[(0, 0)] == [("R", 0, 0, 0), ("R", 1, 0, 0), ("D", 0, 0, 0)]
    assert lists[(0, 1)] == [("R", 0, 0, 1), ("R", 1, 0, 1), ("D", 0, 0, 1)]
    assert lists[(1, 1)] == [("R", 0, 0, 0), ("R", 1, 0, 0), ("C", 0, 0, 0), ("L", 0, 0, 0), ("D", 0, 0, 0)]
    assert lists[(1, 2)] == [("L", 0, 0, 1)]
    assert lists[(2, 2)] == [("L", 0, 0, 0), ("S", 0, 0, 0)]
    # R3 from ground to ground stamps nothing; b: C1's Ieq (subtracted at node 2), L1's iPrev, D1's ieq
    assert lists[(1, n)] == [("C", 0, 1, 1), ("L", 0, 1, 1), ("D", 0, 1, 1)]
    assert lists[(2, n)] == [("L", 0, 1, 0)]
    assert lists[(0, n)] == [("D", 0, 1, 0)]
    # V1 (1 -> 0) at row / column 3, the floating V2 (3 -> 2) at 4: the constant +-1, then the source value in b
    assert lists[(0, 3)] == [("V", -1, 2, 0)] and lists[(3, 0)] == [("V", -1, 2, 0)]
    assert lists[(2, 4)] == [("V", -1, 2, 0)] and lists[(1, 4)] == [("V", -1, 2, 1)]
    assert lists[(4, 2)] == [("V", -1, 2, 0)] and lists[(4, 1)] == [("V", -1, 2, 1)]
    assert lists[(3, n)] == [("V", 0, 0, 0)] and lists[(4, n)] == [("V", 1, 0, 0)]
    assert sorted(lists) == list(lists)  # row-major


def _plan(flat, **kw):
    from emul import pyemul
    opt = abi.SpiceyOptions()
    opt.interpreter = 3
    for k, v in kw.items():
        setattr(opt, k, v)
    info = abi.SpiceyInfo()
    err = C.create_string_buffer(256)
    rc = pyemul.lib().spicey_emul_plan(C.byref(flat.desc()), C.byref(opt), 256, 1, C.byref(info), err, 256)
    return rc, info.as_dict(), err.value.decode()


def test_emulator_plan_reports_exact_mode():
    from spicey_amd import synth
    small = _setup(golden_netlist(load_golden("dchain20")))[0]
    rc, info, _ = _plan(small)
    assert rc == 0 and info["interpreter"] == 3 and info["threads"] == 64 and info["lds_bytes"] > 0
    assert info["n_workgroups"] == 1 and info["wgs_per_inst"] == 1 and info["inst_per_wg"] == 1
    assert info["n_var"] == small.n_var and info["nnz_lu"] == 0 and info["factor_reuse"] == 0 and info["geometry"] == 0
    assert _plan(small, force_global=1)[1]["lds_bytes"] == 0
    assert _plan(small, threads=1024)[1]["threads"] == 1024
    mid = _setup(synth.diode_chain(100, tran=".tran 1e-6 1e-5"))[0]
    rc, info, _ = _plan(mid)
    assert rc == 0 and info["threads"] == 256 and info["lds_bytes"] > 0
    big = _setup(synth.diode_chain(300, tran=".tran 1e-6 1e-5"))[0]
    assert _plan(big)[1]["lds_bytes"] == 0  # beyond the LDS of one CU: the global slab
    # a structurally singular matrix is not refused up front: the reference throws at its first pivot
    assert _plan(_setup(golden_netlist(load_golden("err_singular")))[0])[0] == 0
    for kw, word in ((dict(inst_per_wg=2), "inst_per_wg"), (dict(geometry=1), "geometry"), (dict(front_cut=3), "front_cut"),
                     (dict(wgs_per_inst=2), "wgs_per_inst"), (dict(profile=1), "profile"), (dict(threads=96), "threads")):
        rc, _, err = _plan(small, **kw)
        assert rc == abi.ERR_BAD_DESC and word in err, (kw, err)
