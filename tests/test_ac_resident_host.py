"""CPU twins of tests/test_ac_resident_gpu.py: the same topologies, values, frequencies and phasors (ac_resident_cases.py)
through the emulator's resident sweep (`EmulBackend(ac_resident=True)`: 8 record slots and 2 entries per thread, frequencies
strided by 3) and its per-solve path against the oracle, at the same bars.  They say whether a failure on the device is the
program's or the kernel's, and they check what the device tests presuppose: that the mesh programs have overflow records
and streamed phases and fit the resident capacity, and that the reference alone keeps the random circuits within the
arbitration cap."""
import numpy as np
import pytest

import ac_resident_cases as cases
from ac_resident_cases import cratio, worst
from emul.pyemul import EmulBackend, program_dump, resident_layout
from spicey_amd import abi
from test_ac_batch_host import PerInstanceAcOracle

AC_RMAX, AC_NSE = 12, 10  # kernels.h: record slots and entry slots per thread of the device's resident sweep
HOST_MESH_INST = 5
HOST_LADDER_INST = 8


def reference(oracle_backend, flat, freqs, vph):
    return PerInstanceAcOracle().run_ac(flat, freqs, vph) if np.ndim(vph) == 2 else oracle_backend.run_ac(flat, freqs, vph)


def default_threads(n):
    """AcSparse::upload: threads of the per-solve kernel for n unknowns, and of the resident sweep."""
    T = 64 if n <= 48 else 128 if n <= 160 else 256 if n <= 400 else 1024
    return T, min(T, 512)


def ac_program(flat):
    d = flat.desc()
    d.nS = d.nD = 0
    return program_dump(flat, bank_aware=True, front_cut=0, pcr_top=False, desc=d)[1]


def test_kernel_constants_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(abi.__file__), "csrc", "kernels.h")).read()
    assert int(re.search(r"#define\s+SPICEY_AC_RMAX\s+(\d+)", text).group(1)) == AC_RMAX
    assert int(re.search(r"#define\s+SPICEY_AC_NSE\s+(\d+)", text).group(1)) == AC_NSE


@pytest.mark.parametrize("name", cases.MESHES)
def test_mesh_programs_have_overflow_records_and_streamed_phases(name):
    """What the device test of the meshes relies on: records with more than two products (P.ovf16), at least one phase the
    12 slots of the default geometry cannot hold, and every entry in the 10 entry slots of a thread."""
    flat = cases.ac_only_flat(cases.mesh_text(name))
    full, _, _ = cases.mesh_case(name, 1)
    assert flat.n_nodes == full.n_nodes and flat.n_var == full.n_var <= 66 and flat.nD == flat.nS == 0
    sc = ac_program(flat)
    assert sc["rc"] == 0 and sc["has16"] == 1 and sc["ovf16"] > 0
    T, Tres = default_threads(flat.n_var)
    assert sc["nLU"] <= AC_NSE * Tres
    rc, _, _, ph_cnt, st_cnt, _ = resident_layout(flat, Tres, AC_RMAX, 0)
    assert rc == 0 and (st_cnt > 0).sum() >= 1 and st_cnt.sum() < ph_cnt.sum()


def test_capacity_edge_program_exceeds_64_threads():
    """rlc_mesh(8, 8) with threads=64: more entries than 10 per thread, so the handle keeps the per-solve kernel; the
    default geometry (128 threads) holds them."""
    sc = ac_program(cases.ac_only_flat(cases.mesh_text("rlc8x8")))
    assert AC_NSE * 64 < sc["nLU"] <= AC_NSE * 128


@pytest.mark.parametrize("name", cases.MESHES)
def test_meshes_resident_and_per_solve_vs_oracle(name, oracle_backend):
    flat, freqs, vph = cases.mesh_case(name, HOST_MESH_INST)
    ref = reference(oracle_backend, flat, freqs, vph)
    assert ref["status"] == 0
    one = EmulBackend(1, 64).run_ac(flat, freqs, vph)
    assert one["status"] == 0 and max(worst(one, ref)) <= 1.0, worst(one, ref)
    nLU = ac_program(cases.ac_only_flat(cases.mesh_text(name)))["nLU"]
    first = None
    for T, rev in ((64, False), (512, True), (1024, False)):
        got = EmulBackend(1, T, rev, ac_resident=True).run_ac(flat, freqs, vph)
        assert got["status"] == 0 and max(worst(got, ref)) <= 1.0, (T, worst(got, ref))
        assert max(worst(got, one)) <= 1.0
        # The arithmetic of a task does not depend on T, that of a stamp does: an entry inside the NSE * T entry slots is
        # (gr, w gc) with gc = C1 + C2 summed first, one beyond them w C1 + w C2.  Where every entry is inside (the device's
        # precondition, nLU <= 10 * Tres; here NSE = 2) the bits are those of any other such T.
        if nLU > 2 * T:
            continue
        if first is None:
            first = got
        assert np.array_equal(got["out_v"], first["out_v"]) and np.array_equal(got["out_i"], first["out_i"]), T
    assert nLU <= 2 * 512 and first is not None
    nocur = EmulBackend(1, 512, True, ac_resident=True).run_ac(flat, freqs, vph, want_currents=False)
    assert nocur["status"] == 0 and nocur["out_i"] is None and np.array_equal(nocur["out_v"], first["out_v"])
    if np.ndim(vph) == 2:  # the instances did get phasors of their own
        shared = EmulBackend(1, 512, True, ac_resident=True).run_ac(flat, freqs, vph[0])
        assert np.array_equal(shared["out_v"][0], first["out_v"][0]) and not np.array_equal(shared["out_v"][1], first["out_v"][1])


def test_source_row_beyond_the_first_rows_of_the_workgroup(oracle_backend):
    """fed_ladder(68, 47) with 64 threads: the source's branch equation is pivot row 64, the second row of thread 0 (bit 1 of
    AcResRegs::rowsrc), and the program fits the resident capacity of 64 threads."""
    from emul.pyemul import symbolic
    flat, freqs, vph = cases.fed_ladder_case(HOST_MESH_INST)
    rc, _, rpos, _, _, _ = symbolic(flat)
    assert rc == 0 and flat.nV == 1 and 64 <= rpos[flat.n_nodes] < 128 and flat.n_var == 69
    sc = ac_program(flat)
    assert sc["has16"] == 1 and sc["nLU"] <= AC_NSE * 64
    ref = reference(oracle_backend, flat, freqs, vph)
    assert ref["status"] == 0
    for kw in (dict(ac_resident=True), dict(ac_resident=True, reverse=True), dict()):
        got = EmulBackend(1, 64, **kw).run_ac(flat, freqs, vph)
        assert got["status"] == 0 and max(worst(got, ref)) <= 1.0, (kw, worst(got, ref))


def test_ladder_goes_on_after_a_failed_frequency(oracle_backend):
    """Near-resonant and ordinary frequencies in turn, three frequencies apart in one emulated workgroup: the solve after a
    failed one starts from a clean flag and a freshly stamped workspace; exactly the near slots take the dense fallback."""
    flat, freqs, vph, near = cases.ladder_case(HOST_LADDER_INST)
    assert near.sum(axis=1).tolist() == [3, 1, 0, 0] * (HOST_LADDER_INST // 4)
    ref = oracle_backend.run_ac(flat, freqs, vph)
    assert ref["status"] == 0
    for kw in (dict(ac_resident=True), dict(), dict(ac_resident=True, reverse=True)):
        be = EmulBackend(1, 64, **kw)
        got = be.run_ac(flat, freqs, vph)
        assert got["status"] == 0 and max(worst(got, ref)) <= 1.0, (kw, worst(got, ref))
        assert near.any(axis=1).sum() <= be.info["tail_levels"] <= near.sum(), (kw, be.info["tail_levels"])
        bad = EmulBackend(1, 64, ac_no_dense=True, **kw).run_ac(flat, freqs, vph)
        assert bad["status"] != 0
        assert cratio(bad["out_v"][~near], ref["out_v"][~near]).max() <= 1.0 and cratio(bad["out_i"][~near], ref["out_i"][~near]).max() <= 1.0


_ARBITRATED = {"resident": set(), "per-solve": set(), "reference": set()}


@pytest.mark.parametrize("block", range(4))
def test_random_circuits_with_variants_and_phasors(block, oracle_backend):
    """The 80 random cases of the device test (seeds 0-39 with and without floating sources, 44 instances x 13 frequencies,
    phasors of their own) through both emulator paths.  `reference`: the cases in which the oracle itself is more than one
    budget from the 80-bit solve — these alone must stay within the cap, whatever the kernels do."""
    for seed in range(block * 10, block * 10 + 10):
        for floating in (False, True):
            flat, freqs, vph = cases.random_case(seed, floating)
            ref = PerInstanceAcOracle().run_ac(flat, freqs, vph)
            assert ref["status"] == 0, (seed, floating, ref["detail"])
            if cases.arbitrate(flat, freqs, vph, ref, ref)[0] > 1.0:
                _ARBITRATED["reference"].add((seed, floating))
            for key, be in (("resident", EmulBackend(1, 64, bool(seed & 1), ac_resident=True)), ("per-solve", EmulBackend(1, 64, bool(seed & 1)))):
                got = be.run_ac(flat, freqs, vph)
                assert got["status"] == 0, (seed, floating, key, got["detail"])
                arb, ev, ei = cases.judge_random(flat, freqs, vph, got, ref)
                if arb:
                    _ARBITRATED[key].add((seed, floating))
    for key, seen in _ARBITRATED.items():
        assert len(seen) <= cases.MAX_ARBITRATED, (key, sorted(seen))


def test_one_singular_instance_among_many(oracle_backend):
    n, bad = 9, 4
    flat, freqs, vph, flat_ok, vph_ok = cases.sing_case(n, bad)
    ref = PerInstanceAcOracle().run_ac(flat, freqs, vph)
    assert ref["status"] == abi.ERR_SINGULAR and np.nonzero(ref["inst_status"])[0].tolist() == [bad]
    keep = [k for k in range(n) if k != bad]
    for kw in (dict(ac_resident=True), dict()):
        got = EmulBackend(1, 64, **kw).run_ac(flat, freqs, vph)
        assert got["status"] == abi.ERR_SINGULAR
        alone = EmulBackend(1, 64, **kw).run_ac(flat_ok, freqs, vph_ok)
        assert alone["status"] == 0
        for part in ("out_v", "out_i"):
            a = got[part][keep]
            assert np.isfinite(a.view(np.float64)).all() and np.abs(a).max() > 0
            assert cratio(a, alone[part]).max() <= 1.0 and cratio(a, ref[part][keep]).max() <= 1.0
