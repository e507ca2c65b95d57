"""The packed geometry on its fresh-fill build (program built with fresh_fill, phase B restores the kept entries only, the
first streamed record of factor level 0 in flight under B) against the same handle with SPICEY_NO_FRESH_FILL (default
program, 6-entry build), against the latency geometry — same bits — and against the oracle at the project's bar; with the
phase table and without it.  4 instances x 64 steps per case."""
from __future__ import annotations

import numpy as np
import pytest

from batch_variants import instance
from fresh_host import pyfresh
from test_gpu_parity import tol_ratio
from test_packed_resident_gpu import CASES as PACKED_CASES, STEPS, _chain

pytestmark = pytest.mark.gpu

CASES = dict(PACKED_CASES)
CASES["diode_chain_350"] = lambda: _chain("diode_chain", 350)  # every phase resident: nothing streamed, the fetch under B inactive


def _run(flat, dt, src, geometry):
    from spicey_amd.lib import Handle
    h = Handle(flat, geometry=geometry)
    try:
        r = h.run(STEPS, dt, src)
        assert r["status"] == 0, r["detail"]
        return r, h.info()
    finally:
        h.close()


@pytest.mark.parametrize("no_table", [False, True], ids=["table", "no_table"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fresh_build_same_bits_as_default_build_and_latency_geometry(case, no_table, oracle_backend, monkeypatch):
    if no_table: monkeypatch.setenv("SPICEY_NO_PHASE_TABLE", "1")
    else: monkeypatch.delenv("SPICEY_NO_PHASE_TABLE", raising=False)
    flat, dt, src = CASES[case]()
    assert flat.n_inst == 4
    monkeypatch.delenv("SPICEY_NO_FRESH_FILL", raising=False)
    # (a linear circuit keeps the default program unless told otherwise: here it runs on the fresh build like the others,
    # with the fills of step 0 kept through the reused factorisation)
    monkeypatch.setenv("SPICEY_FRESH_FILL_LINEAR", "1")
    plan = pyfresh.plan(flat, geometry=2)  # (the policy spicey_create runs)
    assert plan["rc"] == 0 and plan["fresh"] == 1 and plan["nKeep"] < plan["nRestore"]
    fresh, info = _run(flat, dt, src, 2)
    latency, info1 = _run(flat, dt, src, 1)
    monkeypatch.setenv("SPICEY_NO_FRESH_FILL", "1")
    assert pyfresh.plan(flat, geometry=2)["fresh"] == 0
    default, info0 = _run(flat, dt, src, 2)
    assert info["geometry"] == 2 and info["threads"] == 512 and info["resident_slots"] == 4 and info1["geometry"] == 1
    for k in ("geometry", "threads", "resident_slots", "streamed_tasks", "resident_tasks", "lds_bytes"):
        assert info0[k] == info[k], k
    for other in (default, latency):
        for k in ("out_v", "out_i", "iters"):
            assert np.array_equal(fresh[k], other[k], equal_nan=(k != "iters")), (case, k)
    if case == "diode_chain_1000":
        assert info["streamed_tasks"] == 2000 and info["resident_tasks"] == 2719
    if case == "diode_chain_350":
        assert info["streamed_tasks"] == 0
    if case == "switched_ladder":
        assert flat.nS > 0 and int(fresh["iters"].max()) > 1
    one = instance(flat, 2)
    ref = oracle_backend.run(one, STEPS, dt, src)
    assert ref["status"] == 0
    assert tol_ratio(fresh["out_v"][2], ref["out_v"][0]).max() <= 1.0 and tol_ratio(fresh["out_i"][2], ref["out_i"][0]).max() <= 1.0
    if flat.nS > 0:
        assert np.array_equal(fresh["iters"][2], ref["iters"][0])
