"""The packed geometry (two 512-thread workgroups per CU, four resident record slots per thread, fresh-fill program, the first
streamed record of factor phase 0 fetched under phase B) on a device beyond chains and ladders: meshes with many streamed
phases of generic records, the bounds of the geometry and of the fresh build, small goldens through the LDS tail levels,
random circuits, batches the launch plan packs by itself, run edges and continuation, and a failing instance.

Every case: the same bits as the same handle options with SPICEY_NO_FRESH_FILL (default program, 6-entry build) and as the
latency geometry — the program's summation order is fixed —, and the oracle at the project's bar (SURVEY.md §8(d):
|x - ref| <= 1e-9 |ref| + 1e-12, integers identical), with the phase table and without it.  Each test prints the share of
that budget it used ("packed-ratio ...") before it asserts."""
from __future__ import annotations

import numpy as np
import pytest

from batch_variants import instance, variant
from conftest import farr, golden_netlist, load_golden
from fresh_host import pyfresh
from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist
from test_gpu_parity import tol_ratio

pytestmark = pytest.mark.gpu

STEPS = 32
TRAN = ".tran 1e-6 7e-5"  # 70 steps: two consecutive runs of STEPS fit
INFO_KEYS = ("geometry", "threads", "resident_slots", "streamed_tasks", "resident_tasks", "lds_bytes")


@pytest.fixture(params=[False, True], ids=["table", "no_table"])
def no_table(request, monkeypatch):
    if request.param: monkeypatch.setenv("SPICEY_NO_PHASE_TABLE", "1")
    else: monkeypatch.delenv("SPICEY_NO_PHASE_TABLE", raising=False)
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL", raising=False)
    monkeypatch.delenv("SPICEY_FRESH_FILL_LINEAR", raising=False)
    return request.param


# ---- circuits -----------------------------------------------------------------------------------------------------------
def _parsed(text):
    ckt = parseNetlist(text)
    dt, steps = abi.computeEffectiveTimeStep(ckt.analyses["tran"]["dt"], ckt.analyses["tran"]["tstop"])
    return ckt, dt, steps


def _spread(flat, n=4):
    """n distinct instances of one topology: R and C scaled per instance, as the switched ladder's batch is."""
    flat = flat.replicate(n)
    for j in range(n):
        flat.R_val[j] *= 1.0 + 0.02 * j
        flat.C_val[j] *= 1.0 - 0.01 * j
    return flat


def _mesh(rows, cols=None):
    ckt, dt, steps = _parsed(synth.rcd_mesh(rows, cols, tran=TRAN))
    return _spread(abi.flatten(ckt)), dt, abi.source_table(ckt, dt, steps)


def _chain(n):
    flat, dt, steps, src = synth.chain_batch("diode_chain", n, [1, 2, 3, 4], tran=TRAN)
    return flat, dt, src


def _golden(name):
    """Four instances of a golden over its own .tran: its text unchanged and variants 1..3 of its R / C / L values (one
    shared source table); replicated with scaled values where a golden has no such value to vary."""
    text = golden_netlist(load_golden(name))
    ckts = [parseNetlist(variant(text, k, amplitude=False)) for k in range(4)]
    ckt, dt, steps = _parsed(text)
    flat = abi.stack_instances([abi.flatten(c) for c in ckts])
    if all(np.array_equal(getattr(flat, k)[0], getattr(flat, k)[1]) for k in ("R_val", "C_val", "L_val")):
        flat = _spread(abi.flatten(ckt))
    return flat, dt, steps, abi.source_table(ckt, dt, steps), ckt


def _run(flat, steps, dt, src, **kw):
    from spicey_amd.lib import Handle
    h = Handle(flat, **kw)
    try:
        r = h.run(steps, dt, src)
        assert r["status"] == 0, r["detail"]
        return r, h.info()
    finally:
        h.close()


def _same_bits(a, b, what):
    for k in ("out_v", "out_i", "iters"):
        assert np.array_equal(a[k], b[k], equal_nan=(k != "iters")), (what, k)


def _meets_oracle(got, j, ref, what):
    """Instance j of a device result against the one-instance oracle result `ref` at the bar, end state included."""
    rv = float(tol_ratio(got["out_v"][j], ref["out_v"][0]).max())
    ri = float(tol_ratio(got["out_i"][j], ref["out_i"][0]).max())
    rs = max(float(tol_ratio(got["state"][k][j], ref["state"][k][0]).max()) for k in ("C_vprev", "L_iprev", "D_vdprev"))
    print(f"packed-ratio {what} inst {j}: out_v {rv:.3g} out_i {ri:.3g} state {rs:.3g}")
    assert np.array_equal(got["iters"][j], ref["iters"][0]), what
    assert rv <= 1.0 and ri <= 1.0 and rs <= 1.0, (what, rv, ri, rs)
    assert np.array_equal(got["state"]["S_ison"][j], ref["state"]["S_ison"][0]), what


def _three_builds(flat, steps, dt, src, monkeypatch, fresh=True):
    """The packed handle as spicey_create plans it, the same options with SPICEY_NO_FRESH_FILL, and the latency geometry:
    the plan's and the handles' facts asserted, the three results bit-equal.  Returns (packed result, plan)."""
    plan = pyfresh.plan(flat, geometry=2)  # (the policy spicey_create runs)
    assert plan["rc"] == 0 and plan["packed"] == 1 and plan["fresh"] == int(fresh), plan
    assert (plan["nKeep"] < plan["nRestore"]) if fresh else (plan["nKeep"] == plan["nRestore"])
    packed, info = _run(flat, steps, dt, src, geometry=2)
    latency, info1 = _run(flat, steps, dt, src, geometry=1)
    monkeypatch.setenv("SPICEY_NO_FRESH_FILL", "1")
    assert pyfresh.plan(flat, geometry=2)["fresh"] == 0
    default, info0 = _run(flat, steps, dt, src, geometry=2)
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL")
    assert info["geometry"] == 2 and info["threads"] == 512 and info["resident_slots"] == 4 and info1["geometry"] == 1
    for k in INFO_KEYS:
        assert info0[k] == info[k] == plan["info"][k], k
    _same_bits(packed, default, "default build")
    _same_bits(packed, latency, "latency geometry")
    return packed, plan


# ---- meshes and bounds --------------------------------------------------------------------------------------------------
# name: (circuit, streamed_tasks, nKeep, nRestore) — what the packing gives today; a change that empties a case shows here
TOPOLOGIES = {
    "rcd_mesh_12": (lambda: _mesh(12), 8082, 166, 1644),        # many streamed phases of generic records, overflow lists, no tridiagonal top
    "rcd_mesh_15": (lambda: _mesh(15), 17188, 266, 2930),       # nRestore just under 6 x 512
    "rcd_mesh_12x20": (lambda: _mesh(12, 20), 16448, 276, 3012),
    "diode_chain_1023": (lambda: _chain(1023), 3070, 1024, 3035),  # nKeep == 2 x 512, n == 2 x 512, more than one streamed phase
    "diode_chain_511": (lambda: _chain(511), 1022, 512, 1503),  # n around the workgroup size
    "diode_chain_512": (lambda: _chain(512), 1024, 513, 1506),
    "diode_chain_513": (lambda: _chain(513), 1026, 514, 1509),
    "diode_chain_2": (lambda: _chain(2), 0, 3, 4),              # 512 threads on almost no work
    "diode_chain_63": (lambda: _chain(63), 0, 64, 171),         # tridiagonal top of 33 .. 35 rows
    "diode_chain_64": (lambda: _chain(64), 0, 65, 174),
    "diode_chain_65": (lambda: _chain(65), 0, 66, 177),
}


@pytest.mark.parametrize("case", sorted(TOPOLOGIES))
def test_meshes_and_bounds(case, no_table, oracle_backend, monkeypatch):
    make, streamed, n_keep, n_restore = TOPOLOGIES[case]
    flat, dt, src = make()
    assert flat.n_inst == 4 and not np.array_equal(flat.R_val[0], flat.R_val[1])
    src = src[: STEPS + 1]
    packed, plan = _three_builds(flat, STEPS, dt, src, monkeypatch)
    assert (plan["info"]["streamed_tasks"], plan["nKeep"], plan["nRestore"]) == (streamed, n_keep, n_restore)
    if case == "diode_chain_1023":
        assert plan["nKeep"] == 2 * 512 and flat.n_var == 2 * 512
    assert not np.array_equal(packed["out_v"][1][-1], packed["out_v"][2][-1])
    ref = oracle_backend.run(instance(flat, 2), STEPS, dt, src)
    assert ref["status"] == 0
    _meets_oracle(packed, 2, ref, case)


@pytest.mark.parametrize("text", [synth.rcd_mesh(16), synth.diode_chain(1024)], ids=["rcd_mesh_16", "diode_chain_1024"])
def test_the_neighbours_beyond_the_bounds_are_refused(text):
    """One more row of mesh, one more link of chain: geometry 2 says so instead of quietly running another geometry."""
    from spicey_amd.lib import Handle, SpiceyNativeError
    flat = abi.flatten(parseNetlist(text)).replicate(4)
    assert pyfresh.plan(flat, geometry=2)["rc"] == abi.ERR_BAD_DESC
    with pytest.raises(SpiceyNativeError, match="geometry 2 needs") as e:
        Handle(flat, geometry=2).close()
    assert e.value.status == abi.ERR_BAD_DESC


# ---- goldens through the tail path ----------------------------------------------------------------------------------------
GOLDENS = ["boost_probe", "half_bridge", "diode_switch", "switch_vt_vh", "vswitch_pwl", "relay_osc", "star_hub", "bridge_bleed", "dchain20", "mesh9x5"]
# the goldens with switches whose switch flips within the golden's own .tran (boost_probe's never does: the reference itself
# reports one iteration on every step of it, and so must the device)
ITERATING = ("half_bridge", "diode_switch", "switch_vt_vh", "vswitch_pwl", "relay_osc")


def _capped(ref, steps):
    """Index of the reference's first step at its 20-iteration cap."""
    capped = np.nonzero(ref["iters"][0] >= 20)[0]
    return int(capped[0]) if len(capped) else steps + 1


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_through_the_tail_levels(name, no_table, oracle_backend, monkeypatch):
    """relay_osc sits at the reference's 20-iteration cap from step 0 on, so "everything before the first capped step"
    (test_gpu_parity.py::test_skipped_random_seeds_arbitrated_on_gpu) is nothing there.  It has no memory and its switch
    sees 5 mV or 5 V against a threshold of 2.5 V, so nothing hangs on a last bit: it is compared in full, like the others
    (and like test_hip_vs_oracle_and_golden does on the default path)."""
    flat, dt, steps, src, ckt = _golden(name)
    assert flat.n_inst == 4 and any(not np.array_equal(getattr(flat, k)[0], getattr(flat, k)[2]) for k in ("R_val", "C_val", "L_val"))
    packed, plan = _three_builds(flat, steps, dt, src, monkeypatch)
    assert plan["info"]["streamed_tasks"] == 0 and plan["info"]["tail_levels"] > 0
    assert (int(packed["iters"].max()) > 1) == (name in ITERATING) and (name not in ITERATING or flat.nS > 0)
    for j in (0, 2):
        ref = oracle_backend.run(instance(flat, j), steps, dt, src)
        assert ref["status"] == 0
        assert (_capped(ref, steps) <= steps) == (name == "relay_osc")
        _meets_oracle(packed, j, ref, f"golden {name}")
    run = load_golden(name)["runs"][0]  # instance 0 is the text unchanged: the reference's own recorded numbers
    for k in run["keysV"]:
        col = ckt.nodes.rev.index(k) - 1
        assert tol_ratio(packed["out_v"][0][:, col], farr(run["V"][k])).max() <= 1.0, (name, k)


@pytest.mark.parametrize("name", ["lc_tank", "fv_chain"])
def test_a_linear_golden_keeps_the_default_program(name, no_table, oracle_backend, monkeypatch):
    """Factor reuse leaves the fresh class nothing to save: the packed default program, the latency geometry's bits."""
    flat, dt, steps, src, _ = _golden(name)
    packed, plan = _three_builds(flat, steps, dt, src, monkeypatch, fresh=False)
    assert plan["program_fresh_fill"] == 0
    ref = oracle_backend.run(instance(flat, 2), steps, dt, src)
    assert ref["status"] == 0
    _meets_oracle(packed, 2, ref, f"golden {name}")


# ---- random circuits ------------------------------------------------------------------------------------------------------
# left out, as in test_gpu_parity.py::test_random_circuits_on_gpu (six seeds at the reference's iteration cap, three whose
# fp64 conditioning leaves no margin; test_skipped_random_seeds_arbitrated_on_gpu runs them)
RANDOM_SKIP = {36, 116, 117, 182, 185, 192, 59, 76, 190}
BLOCK = 20
_RANDOM: dict = {}


def _random_case(seed, floating):
    """(flat of one instance, dt, steps, src, oracle result), computed once per seed and never modified."""
    key = (seed, floating)
    if key not in _RANDOM:
        from oracle.pyoracle import OracleBackend
        from random_circuits import random_netlist
        ckt, dt, steps = _parsed(random_netlist(seed, floating_sources=floating))
        flat = abi.flatten(ckt)
        src = abi.source_table(ckt, dt, steps)
        ref = OracleBackend().run(flat, steps, dt, src)
        for a in (ref["out_v"], ref["out_i"], ref["iters"]):
            a.setflags(write=False)
        _RANDOM[key] = (flat, dt, steps, src, ref)
    return _RANDOM[key]


def _kept(floating):
    """The seeds the twin tests of the default path keep: a condition on the reference's run, not a measurement."""
    if not floating:
        return [s for s in range(200) if s not in RANDOM_SKIP]
    out = []
    for s in range(120):
        ref = _random_case(s, True)[4]
        if ref["status"] == 0 and ref["iters"].max() < 20:
            out.append(s)
    return out


def _hp_bar(v, flat, steps, dt, src, ref):
    """(v's distance, the fp64 reference's own distance) from the 80-bit replay, in budgets (test_gpu_parity.py, the
    floating-source twin: one budget, absolute part scaled by the run's largest voltage)."""
    import hp_reference
    hp, _ = hp_reference.run(flat, steps, dt, src)
    tol = 1e-9 * np.abs(hp) + 1e-12 * max(1.0, float(np.nanmax(np.abs(ref["out_v"]))))
    return float((np.abs(v - hp) / tol).max()), float((np.abs(ref["out_v"][0] - hp) / tol).max())


def _budget_used(got, j, ref):
    """The largest share of the bar instance j of `got` uses against the one-instance oracle result: voltages, the currents
    that are finite in the reference, end state."""
    fin = np.isfinite(ref["out_i"][0])
    if not np.array_equal(fin, np.isfinite(got["out_i"][j])):
        return np.inf
    return max(float(tol_ratio(got["out_v"][j], ref["out_v"][0]).max()), float(tol_ratio(got["out_i"][j][fin], ref["out_i"][0][fin]).max()),
               *(float(tol_ratio(got["state"][k][j], ref["state"][k][0]).max()) for k in ("C_vprev", "L_iprev", "D_vdprev")))


def _check_random_seed(seed, floating):
    """One seed, two instances, geometry 2: the latency geometry's bits and the oracle at the bar.  First on the CPU: the
    packed emulation of the same program meets the oracle at that bar, or the seed is arbitrated in extended precision
    (both the emulation and the device: one budget from the 80-bit replay, or four times the reference's own distance)."""
    flat, dt, steps, src, ref = _random_case(seed, floating)
    what = f"random {seed}{' floating' if floating else ''}"
    two = flat.replicate(2)
    assert pyfresh.plan(two, geometry=2)["packed"] == 1, what
    emu = pyfresh.run(flat, steps, dt, src, fresh=True)
    assert emu["status"] == 0 and np.array_equal(emu["iters"], ref["iters"]), what
    arbitrate = _budget_used(emu, 0, ref) > 1.0
    if arbitrate:
        e_emu, e_ref = _hp_bar(emu["out_v"][0], flat, steps, dt, src, ref)
        assert e_emu <= max(1.0, 4.0 * e_ref), (what, e_emu, e_ref)
    packed, info = _run(two, steps, dt, src, geometry=2)
    latency, _ = _run(two, steps, dt, src, geometry=1)
    assert info["geometry"] == 2 and info["threads"] == 512 and info["resident_slots"] == 4
    _same_bits(packed, latency, what)
    assert np.array_equal(packed["out_v"][0], packed["out_v"][1]) and np.array_equal(packed["iters"][1], ref["iters"][0]), what
    assert np.array_equal(packed["state"]["S_ison"][1], ref["state"]["S_ison"][0]), what
    if arbitrate:
        e_dev, e_ref = _hp_bar(packed["out_v"][1], flat, steps, dt, src, ref)
        print(f"packed-ratio {what} ARBITRATED: device {e_dev:.3g} reference {e_ref:.3g} budgets from the 80-bit replay")
        assert e_dev <= max(1.0, 4.0 * e_ref), (what, e_dev, e_ref)
        return 0.0
    worst = _budget_used(packed, 1, ref)
    if worst > 0.5: print(f"packed-ratio {what}: {worst:.3g}")
    assert worst <= 1.0, (what, worst)
    return worst


@pytest.mark.parametrize("floating,block", [(False, b) for b in range(200 // BLOCK)] + [(True, b) for b in range(120 // BLOCK)],
                         ids=lambda v: {False: "grounded", True: "floating"}[v] if isinstance(v, bool) else f"seeds_{v * BLOCK}")
def test_random_circuits(floating, block, no_table):
    kept = _kept(floating)
    assert len(kept) == 191 if not floating else len(kept) >= 100  # (what the twin tests assert as `ran`)
    seeds = [s for s in kept if block * BLOCK <= s < (block + 1) * BLOCK]
    assert seeds
    worst = max(_check_random_seed(s, floating) for s in seeds)
    print(f"packed-ratio random {'floating' if floating else 'grounded'} seeds {seeds[0]}..{seeds[-1]}: {len(seeds)} ran, worst {worst:.3g}")


# ---- two workgroups on one CU, chosen by the launch plan -----------------------------------------------------------------
N_AUTO = 520


def _auto_batch(flat, dt, src, steps, oracle_backend, what):
    flat = flat.replicate(N_AUTO)
    flat.R_val *= np.linspace(1.0, 1.3, N_AUTO)[:, None]
    src = src[: steps + 1]
    auto, info = _run(flat, steps, dt, src)  # no geometry option
    assert info["geometry"] == 2 and info["n_workgroups"] == N_AUTO and info["threads"] == 512 and info["resident_slots"] == 4
    latency, info1 = _run(flat, steps, dt, src, geometry=1)
    assert info1["geometry"] == 1
    _same_bits(auto, latency, what)
    assert len({auto["out_v"][i, -1].tobytes() for i in range(N_AUTO)}) == N_AUTO  # no instance answers for another
    for j in (0, 255, 256, 257, 519):
        ref = oracle_backend.run(instance(flat, j), steps, dt, src)
        assert ref["status"] == 0
        _meets_oracle(auto, j, ref, what)
    return auto


def test_520_meshes_take_the_packed_geometry_by_themselves(no_table, oracle_backend):
    ckt, dt, steps = _parsed(synth.rcd_mesh(12, tran=TRAN))
    _auto_batch(abi.flatten(ckt), dt, abi.source_table(ckt, dt, steps), 8, oracle_backend, "520 x rcd_mesh_12")


def test_520_half_bridges_take_the_packed_geometry_by_themselves(no_table, oracle_backend):
    text = golden_netlist(load_golden("half_bridge"))
    ckt, dt, steps = _parsed(text)
    auto = _auto_batch(abi.flatten(ckt), dt, abi.source_table(ckt, dt, steps), steps, oracle_backend, "520 x half_bridge")
    assert int(auto["iters"].max()) > 1


# ---- run edges and continuation -------------------------------------------------------------------------------------------
EDGE_CASES = {"diode_chain_1000": lambda: _chain(1000), "rcd_mesh_12": lambda: _mesh(12)}


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_runs_of_no_step_and_of_one_step(case, no_table):
    """Nothing to fetch past the end: the record fetch under B and the source prefetch of the "next" step."""
    flat, dt, src = EDGE_CASES[case]()
    full, info = _run(flat, STEPS, dt, src[: STEPS + 1], geometry=2)
    assert info["geometry"] == 2 and info["streamed_tasks"] > 0
    for steps in (0, 1):
        short, _ = _run(flat, steps, dt, src[: steps + 1], geometry=2)
        assert short["status"] == 0
        for k in ("out_v", "out_i", "iters"):
            assert short[k].shape[1] == steps + 1
            assert np.array_equal(short[k], full[k][:, : steps + 1], equal_nan=(k != "iters")), (case, steps, k)


def _same_state(a, b, what):
    for k in ("C_vprev", "L_iprev", "D_vdprev", "S_ison"):
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_continuation_set_state_and_reset(case, no_table):
    from spicey_amd.lib import Handle
    flat, dt, src = EDGE_CASES[case]()
    src1, src2 = src[: STEPS + 1], src[STEPS: 2 * STEPS + 1]
    assert len(src2) == STEPS + 1
    p, q, l = Handle(flat, geometry=2), Handle(flat, geometry=2), Handle(flat, geometry=1)
    try:
        assert p.info()["geometry"] == q.info()["geometry"] == 2 and l.info()["geometry"] == 1
        p1, l1 = p.run(STEPS, dt, src1), l.run(STEPS, dt, src1)
        kept = p.state()
        p2, l2 = p.run(STEPS, dt, src2), l.run(STEPS, dt, src2)
        for a, b, what in ((p1, l1, "run 1"), (p2, l2, "run 2")):
            assert a["status"] == b["status"] == 0
            _same_bits(a, b, (case, what))
            _same_state(a["state"], b["state"], (case, what))
        assert not np.array_equal(p1["out_v"], p2["out_v"]) and not np.array_equal(p1["state"]["C_vprev"], p2["state"]["C_vprev"])
        _same_state(kept, p1["state"], (case, "get_state"))
        q.set_state(kept)  # the state after run 1 on a new packed handle: run 2 again
        q2 = q.run(STEPS, dt, src2)
        assert q2["status"] == 0
        _same_bits(q2, p2, (case, "set_state"))
        _same_state(q2["state"], p2["state"], (case, "set_state"))
        p.reset_state()
        assert p.sync() == 0
        again = p.run(STEPS, dt, src1)
        assert again["status"] == 0
        _same_bits(again, p1, (case, "reset"))
        _same_state(again["state"], p1["state"], (case, "reset"))
    finally:
        for h in (p, q, l):
            h.close()


# ---- a failing instance ---------------------------------------------------------------------------------------------------
def _isolate_a_node(flat, j):
    """Instance j with one mesh node cut off: its resistors 1e16 ohm, its capacitor 1e-30 F, no diode there — the node's
    pivot falls below the reference's 1e-15."""
    on_diode = set(flat.D_np) | set(flat.D_nm) | set(flat.V_n1) | set(flat.V_n2)
    node = next(u for u in range(flat.n_nodes // 2, flat.n_nodes) if u not in on_diode)
    flat.R_val[j, (flat.R_n1 == node) | (flat.R_n2 == node)] = 1e16
    flat.C_val[j, (flat.C_n1 == node) | (flat.C_n2 == node)] = 1e-30
    return node


def test_a_singular_instance_in_a_packed_fresh_batch(no_table, oracle_backend):
    from spicey_amd.lib import Handle
    healthy, dt, src = _mesh(12)
    src = np.ascontiguousarray(np.broadcast_to(src[: STEPS + 1], (4, STEPS + 1, healthy.nV)))  # (per-instance layout: partial results stand)
    broken, _, _ = _mesh(12)
    _isolate_a_node(broken, 2)
    assert oracle_backend.run(instance(broken, 2), STEPS, dt, src[2])["status"] == abi.ERR_SINGULAR
    assert oracle_backend.run(instance(healthy, 2), STEPS, dt, src[2])["status"] == 0
    plan = pyfresh.plan(broken, geometry=2)
    assert plan["packed"] == 1 and plan["fresh"] == 1 and plan["info"]["streamed_tasks"] == 8082
    good, info = _run(healthy, STEPS, dt, src, geometry=2)
    h = Handle(broken, geometry=2)
    try:
        bad = h.run(STEPS, dt, src)
        assert h.info()["geometry"] == 2
    finally:
        h.close()
    assert bad["status"] == abi.ERR_SINGULAR and bad["partial"]
    assert np.array_equal(bad["inst_status"], [0, 0, abi.ERR_SINGULAR, 0])
    for j in (0, 1, 3):
        for k in ("out_v", "out_i", "iters"):
            assert np.array_equal(bad[k][j], good[k][j], equal_nan=(k != "iters")), (j, k)
        _same_state({k: v[j] for k, v in bad["state"].items()}, {k: v[j] for k, v in good["state"].items()}, j)
