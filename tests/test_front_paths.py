"""Which path of the dense-front engine (spicey_amd/csrc/fronts_exec.h) every front of tests/front_cases.py takes — asked
of the engine's own predicates through the emulator's build of it (emul.pyemul.front_census), never restated here — and
the CPU twin of tests/test_front_paths_gpu.py: the same cases through the host form of the same code against the oracle.
A case that fails here fails in the program (symbolic phase, schedule, the arithmetic both forms share); one that passes
here and fails on the device fails in the text only the device compiles."""
import numpy as np
import pytest

import front_cases as fc
from emul.pyemul import EmulBackend, front_census
from test_program_emul import ratio

CASES = list(fc.SHAPES)


def census(name, G=1):
    c = front_census(fc.case(name).flat, fc.FRONT_CUT, G)
    c["panels"] = c["Pp"] // 16
    c["staged"] = 1 - c["fits_lds"]  # by size: with the product's LDS budget
    return c


def test_the_cases_hold_every_class_of_front():
    """Every class of front the device tests are meant to reach occurs in at least one case.  `staged` is by size (the
    product's LDS budget); tile columns and waves are those of trailing_left_cols at the 512 threads of the full-size
    mesh's launch, which the device tests ask for in two of their variants (front_cases.THREADS; the others run the 256
    the plan picks for circuits of this size)."""
    found = {k: [] for k in "a b c d e f_out f_in g_few g_many h_staged h_lds levels".split()}
    for name in CASES:
        c = census(name)
        plan = fc.cpu_plan(fc.case(name).flat, force_global=1, wgs_per_inst=2, threads=fc.THREADS, front_cut=fc.FRONT_CUT)
        assert plan["threads"] == fc.THREADS and plan["n_fronts"] == c["n_fronts"] and c["front_cut"] == fc.FRONT_CUT
        waves = plan["threads"] // 64
        for f in range(c["n_fronts"]):
            g = {k: int(c[k][f]) for k in c if isinstance(c[k], np.ndarray)}
            lds, staged, root = g["fits_lds"] == 1, g["staged"] == 1, g["parent"] < 0
            left = staged and g["left_fits"] == 1
            tile_cols = (g["Mp"] - g["Pp"]) // 16 + 1  # the boundary's tile columns and the right-hand side's
            hit = dict(a=lds and g["panels"] >= 3 and g["q"] > 0 and g["Mp"] == 128,
                       b=lds and root and g["stays_in_lds"] == 1 and g["panels"] >= 5,
                       c=left and g["panels"] >= 6 and g["q"] > 0,
                       d=staged and not left,
                       e=staged and root and g["q"] == 0 and g["panels"] >= 9,
                       f_out=staged and g["rows_fit"] == 0, f_in=staged and g["rows_fit"] == 1,
                       g_few=left and g["q"] > 0 and tile_cols < waves, g_many=left and g["q"] > 0 and tile_cols >= waves,
                       h_staged=not root and staged and c["staged"][g["parent"]] == 1,
                       h_lds=not root and staged and c["fits_lds"][g["parent"]] == 1,
                       levels=not root and staged and g["children"] > 0 and c["parent"][g["parent"]] < 0)
            for k, v in hit.items():
                if v:
                    found[k].append((name, g["p"], g["q"]))
        # under stage_fronts=True nothing above 64 rows stays in LDS, and the case has such fronts
        assert ((c["fits_lds_staged"] == 1) <= (c["Mp"] <= 64)).all() and (c["fits_lds_staged"] == 0).any()
        assert (c["fits_lds_staged"] <= c["fits_lds"]).all() and (c["rows_fit_staged"] <= c["rows_fit"]).all()
    missing = [k for k, v in found.items() if not v]
    assert not missing, (missing, found)


@pytest.mark.parametrize("name", CASES)
def test_the_host_form_agrees_with_the_oracle(name, oracle_backend, monkeypatch):
    """The case through the emulator with fronts: the oracle's iteration counts and the parity bar on voltages, currents and
    end state; the same bits with the fronts LDS-resident and staged, left- and right-looking, in both thread orders; and
    no factorisation is reused (the circuit is nonlinear: every solve refactors)."""
    c = fc.case(name)
    ref = fc.oracle_ref(c, oracle_backend)
    assert ref["status"] == 0 and c.flat.nD > 0 and c.steps <= 8 and c.flat.n_var <= 260
    assert fc.cpu_plan(c.flat, force_global=1, wgs_per_inst=1, front_cut=fc.FRONT_CUT)["factor_reuse"] == 0
    first = None
    for right in (False, True):
        if right:
            monkeypatch.setenv("SPICEY_FRONT_RIGHT_LOOKING", "1")
        for rev in (False, True):
            for stage in (False, True):
                be = EmulBackend(1, 512, rev, front_cut=fc.FRONT_CUT, stage_fronts=stage)
                got = be.run(c.flat, c.steps, c.dt, c.src)
                key = (right, rev, stage)
                assert got["status"] == 0 and be.info["tail_levels"] == census(name)["n_fronts"], key  # (tail_levels carries the front count here)
                assert np.array_equal(got["iters"], ref["iters"]), key
                assert be.solves == int(ref["iters"].sum()), key  # one factorisation and solve per Newton iteration
                if first is None:
                    first = got
                    assert ratio(got["out_v"], ref["out_v"]).max() <= 1.0 and ratio(got["out_i"], ref["out_i"]).max() <= 1.0
                    for k in ("C_vprev", "D_vdprev"):
                        assert ratio(got["state"][k], ref["state"][k]).max() <= 1.0, k
                assert np.array_equal(got["out_v"], first["out_v"]) and np.array_equal(got["out_i"], first["out_i"]), key
                for k in ("C_vprev", "D_vdprev"):
                    assert np.array_equal(got["state"][k], first["state"][k]), (key, k)


def test_a_floating_pair_in_a_staged_front_is_singular(oracle_backend):
    """The singular case of the device tests: the oracle's verdict, and the emulator's through a staged multi-panel front."""
    name, r = fc.FLOATING
    bad = fc.case(name).reseeded(5, floating_pair=r)
    ok = fc.case(name).reseeded(5, floating_pair=1e3)
    cen = front_census(bad.flat, fc.FRONT_CUT)
    assert ((cen["fits_lds"] == 0) & (cen["Pp"] >= 32) & (cen["q"] > 0)).any()
    assert np.array_equal(front_census(ok.flat, fc.FRONT_CUT)["p"], cen["p"])  # (one topology: the values alone differ)
    from spicey_amd import abi
    assert oracle_backend.run(bad.flat, bad.steps, bad.dt, bad.src)["status"] == abi.ERR_SINGULAR
    assert oracle_backend.run(ok.flat, ok.steps, ok.dt, ok.src)["status"] == 0
    for stage in (False, True):
        assert EmulBackend(1, 512, front_cut=fc.FRONT_CUT, stage_fronts=stage).run(bad.flat, bad.steps, bad.dt, bad.src)["status"] == abi.ERR_SINGULAR
        assert EmulBackend(1, 512, front_cut=fc.FRONT_CUT, stage_fronts=stage).run(ok.flat, ok.steps, ok.dt, ok.src)["status"] == 0
