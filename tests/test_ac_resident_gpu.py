"""Device tests of the AC resident sweep (`spicey_ac_kernel_res<12, 10>`) beyond ladders: meshes (overflow records, streamed
phases), the capacity edge, a workgroup that goes on after a failed frequency with the dense fallback behind it, random
circuits, and one singular instance among many — every batch with more than 512 (instance, frequency) slots, every test
asserting which kernel ran.  Bar: |z - z_ref| <= 1e-9 |z_ref| + 1e-12 against the oracle.  Inputs and
tolerances are those of the CPU twins in test_ac_resident_host.py (ac_resident_cases.py)."""
import time

import numpy as np
import pytest

import ac_resident_cases as cases
from ac_resident_cases import cratio, worst
from spicey_amd import abi
from test_ac_batch_host import PerInstanceAcOracle

pytestmark = pytest.mark.gpu


def reference(oracle_backend, flat, freqs, vph):
    return PerInstanceAcOracle().run_ac(flat, freqs, vph) if np.ndim(vph) == 2 else oracle_backend.run_ac(flat, freqs, vph)


def sweep(flat, freqs, vph, want_currents=True, **kw):
    """(result, info) of one sweep on a handle of its own."""
    from spicey_amd.lib import AcHandle
    h = AcHandle(flat, **kw)
    got = h.run(freqs, vph, want_currents)
    info = h.info()
    h.close()
    return got, info


@pytest.mark.parametrize("name", cases.MESHES)
def test_meshes_in_the_resident_kernel(name, oracle_backend):
    """34 variants x 16 frequencies of a mesh: records with more than two products and streamed phases in the default
    geometry; the bits do not depend on the thread count, nor the voltages on whether currents are recorded."""
    t0 = time.perf_counter()
    flat, freqs, vph = cases.mesh_case(name)
    assert flat.n_inst * len(freqs) > 512 and flat.n_var <= 66
    ref = reference(oracle_backend, flat, freqs, vph)
    assert ref["status"] == 0
    got, info = sweep(flat, freqs, vph)
    assert got["status"] == 0, got["detail"]
    assert info["interpreter"] == 2 and info["resident_tasks"] > 0 and info["streamed_tasks"] > 0, info
    ev, ei = worst(got, ref)
    print(f"{name}: resident {ev:.3g} / {ei:.3g} of the bar, resident_tasks {info['resident_tasks']}, streamed_tasks {info['streamed_tasks']}, threads {info['threads']}")
    assert ev <= 1.0 and ei <= 1.0
    one, info1 = sweep(flat, freqs, vph, no_resident=True)
    assert one["status"] == 0 and info1["interpreter"] == 1
    print(f"{name}: per-solve {worst(one, ref)}, resident against per-solve {worst(got, one)}")
    assert max(worst(one, ref)) <= 1.0 and max(worst(got, one)) <= 1.0
    for threads in (256, 512, 1024):
        g, i = sweep(flat, freqs, vph, threads=threads)
        assert g["status"] == 0 and i["interpreter"] == 2 and i["resident_tasks"] > 0 and i["threads"] == threads
        assert max(worst(g, ref)) <= 1.0
        assert np.array_equal(g["out_v"], got["out_v"]) and np.array_equal(g["out_i"], got["out_i"]), threads
    nocur, i = sweep(flat, freqs, vph, want_currents=False)
    assert nocur["status"] == 0 and i["interpreter"] == 2 and nocur["out_i"] is None and np.array_equal(nocur["out_v"], got["out_v"])
    print(f"{name}: {time.perf_counter() - t0:.2f} s")


def test_capacity_edge_keeps_the_per_solve_kernel(oracle_backend):
    """rlc_mesh(8, 8) with 64 threads: ~750 entries against 10 x 64 entry slots — the handle has no resident layout, and a
    batch that outnumbers the CUs runs the per-solve kernel."""
    t0 = time.perf_counter()
    flat, freqs, vph = cases.mesh_case("rlc8x8")
    assert flat.n_inst * len(freqs) > 512
    ref = reference(oracle_backend, flat, freqs, vph)
    got, info = sweep(flat, freqs, vph, threads=64)
    assert got["status"] == 0 and info["interpreter"] == 1 and info["threads"] == 64 and info["nnz_lu"] > 640, info
    print(f"capacity edge: nnz_lu {info['nnz_lu']}, {worst(got, ref)} of the bar, {time.perf_counter() - t0:.2f} s")
    assert max(worst(got, ref)) <= 1.0


def test_source_row_beyond_the_first_rows_of_the_workgroup(oracle_backend):
    """fed_ladder(68, 47) with 64 threads stays resident (~300 entries) and has its only right-hand side in pivot row 64: the
    second row of thread 0 (bit 1 of AcResRegs::rowsrc), with a phasor of its own for every instance."""
    t0 = time.perf_counter()
    flat, freqs, vph = cases.fed_ladder_case()
    assert flat.n_inst * len(freqs) > 512
    ref = reference(oracle_backend, flat, freqs, vph)
    assert ref["status"] == 0
    got, info = sweep(flat, freqs, vph, threads=64)
    assert got["status"] == 0, got["detail"]
    assert info["interpreter"] == 2 and info["threads"] == 64 and info["n_var"] == 69, info
    print(f"fed ladder: resident {worst(got, ref)} of the bar, resident_tasks {info['resident_tasks']}, streamed_tasks {info['streamed_tasks']}")
    assert max(worst(got, ref)) <= 1.0
    one, info1 = sweep(flat, freqs, vph, threads=64, no_resident=True)
    assert one["status"] == 0 and info1["interpreter"] == 1 and max(worst(one, ref)) <= 1.0 and max(worst(got, one)) <= 1.0
    print(f"fed ladder: {time.perf_counter() - t0:.2f} s")


def test_workgroup_goes_on_after_a_failed_frequency_and_dense_fallback(oracle_backend):
    """520 instances x 9 frequencies: one workgroup runs all frequencies of its instance, near-resonant and ordinary ones
    in turn.  The near slots (and no others) are repeated by the dense kernel behind the resident sweep; without it they
    fail and every other slot is still right — the flag and the workspace of a failed solve do not reach the next."""
    t0 = time.perf_counter()
    flat, freqs, vph, near = cases.ladder_case()
    assert flat.n_inst == 520
    ref = oracle_backend.run_ac(flat, freqs, vph)
    assert ref["status"] == 0
    got, info = sweep(flat, freqs, vph)
    assert got["status"] == 0, got["detail"]
    assert info["interpreter"] == 2
    print(f"ladder: {worst(got, ref)} of the bar, dense solves {info['tail_levels']} (instances with a near slot {near.any(axis=1).sum()}, near slots {near.sum()})")
    assert max(worst(got, ref)) <= 1.0
    assert near.any(axis=1).sum() <= info["tail_levels"] <= near.sum()
    bad, info = sweep(flat, freqs, vph, no_dense=True)
    assert bad["status"] != 0 and info["interpreter"] == 2 and info["tail_levels"] == 0
    ev, ei = cratio(bad["out_v"][~near], ref["out_v"][~near]).max(), cratio(bad["out_i"][~near], ref["out_i"][~near]).max()
    print(f"ladder without the fallback: status {bad['status']}, slots that are not near {ev:.3g} / {ei:.3g} of the bar, {time.perf_counter() - t0:.2f} s")
    assert ev <= 1.0 and ei <= 1.0
    assert set(np.nonzero(bad["inst_status"])[0]) <= set(np.nonzero(near.any(axis=1))[0])


_ARBITRATED = {"resident": set(), "per-solve": set()}


@pytest.mark.parametrize("block", range(4))
def test_random_circuits_on_the_device(block, oracle_backend):
    """Seeds block*10 .. block*10+9 with and without floating sources, 44 instances (variants 0-7 in turn, see
    ac_resident_cases.random_case) x 13 frequencies each with phasors of their own, through the resident sweep and the
    per-solve kernel.  At most 3 of the 80 cases per kernel may rest on the 80-bit arbitration (counted over the blocks run
    so far), none is skipped."""
    t0 = time.perf_counter()
    wv = wi = 0.0
    dense = 0
    for seed in range(block * 10, block * 10 + 10):
        for floating in (False, True):
            flat, freqs, vph = cases.random_case(seed, floating)
            assert flat.n_inst * len(freqs) > 512
            ref = PerInstanceAcOracle().run_ac(flat, freqs, vph)
            assert ref["status"] == 0, (seed, floating, ref["detail"])
            for key, kw, mode in (("resident", dict(), 2), ("per-solve", dict(no_resident=True), 1)):
                got, info = sweep(flat, freqs, vph, **kw)
                assert got["status"] == 0, (seed, floating, key, got["detail"])
                assert info["interpreter"] == mode, (seed, floating, key, info)
                dense += info["tail_levels"]
                arb, ev, ei = cases.judge_random(flat, freqs, vph, got, ref)
                if arb:
                    _ARBITRATED[key].add((seed, floating))
                    print(f"arbitrated: seed {seed} floating {floating} {key}: {ev:.3g} of the voltage budget")
                else:
                    wv, wi = max(wv, ev), max(wi, ei)
    print(f"block {block}: worst {wv:.3g} / {wi:.3g} of the budget, dense solves {dense}, arbitrated so far {({k: sorted(v) for k, v in _ARBITRATED.items()})}, {time.perf_counter() - t0:.2f} s")
    for key, seen in _ARBITRATED.items():
        assert len(seen) <= cases.MAX_ARBITRATED, (key, sorted(seen))


def test_one_singular_instance_in_the_resident_sweep():
    """Instance 257 of 520 carries the values of ac_sing_first (a node floats at the first frequency): the sweep names it
    and it alone, and the rows of the other 519 are those of a batch without it."""
    t0 = time.perf_counter()
    flat, freqs, vph, flat_ok, vph_ok = cases.sing_case()
    bad = cases.SING_AT
    got, info = sweep(flat, freqs, vph)
    assert info["interpreter"] == 2
    assert got["status"] == abi.ERR_SINGULAR and f"inst {bad} frequency index 0" in got["detail"], got["detail"]
    assert np.nonzero(got["inst_status"])[0].tolist() == [bad] and got["first_freq"][bad] == 0
    assert (np.delete(got["first_freq"], bad) == -1).all()
    rest, info = sweep(flat_ok, freqs, vph_ok)
    assert rest["status"] == 0 and info["interpreter"] == 2 and not rest["inst_status"].any()
    keep = [k for k in range(flat.n_inst) if k != bad]
    for part in ("out_v", "out_i"):
        a = got[part][keep]
        assert np.isfinite(a.view(np.float64)).all() and np.abs(a).max() > 0
        e = cratio(a, rest[part]).max()
        print(f"singular instance: {part} of the others {e:.3g} of the bar")
        assert e <= 1.0
    print(f"singular instance: {time.perf_counter() - t0:.2f} s")
