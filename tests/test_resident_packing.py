"""Register-resident packing (spicey_build_resident): as few streamed phases as possible, then as few streamed tasks.

A streamed phase costs one exposed L2 round trip per solve whatever its size, so a phase that does not fit the slots in its
generic form is tried as row records (two consecutive slots per chunk) wherever two slots of a wave are free, and chunks go
where there is room instead of only at the round-robin cursor.  Every layout that differs from the one the previous packing
rule gave must stream fewer phases; tests/golden/resident_layout_parent.json holds what that rule gave (streamed phases,
streamed tasks and a digest of the slot table per case, recorded from the commit before this packing, not from this code).
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np
import pytest

from spicey_amd import abi, synth
from spicey_amd.netlist import parseNetlist

from emul.pyemul import EmulBackend, resident_layout, row_record_counts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resident_layout_parent.json")
GEOMETRIES = ((128, 4), (256, 4), (512, 4), (512, 16), (1024, 8))
# (tridiagonal top, longest tail, row records): what the transient plan asks for, with and without row records, and the
# plain task lists of the AC resident sweep (generic records only)
PROGRAMS = ((True, 24, False), (True, 24, True), (False, 0, False))


def circuits():
    for n in range(100, 1201, 50):
        yield f"diode_chain({n})", synth.diode_chain(n)
        yield f"rc_ladder({n})", synth.rc_ladder(n)
    for rows in (6, 12, 20):
        yield f"rcd_mesh({rows})", synth.rcd_mesh(rows)


def layout_record(flat, T, rmax, max_tail, pcr_top, row_records):
    rc, res_phase, res_valid, ph_cnt, st_cnt, meta = resident_layout(flat, T, rmax, max_tail, pcr_top=pcr_top, row_records=row_records)
    assert rc == 0
    return {"res_phase": res_phase, "res_valid": res_valid, "ph_cnt": ph_cnt, "st_cnt": st_cnt, "meta": meta,
            "streamed_phases": int((st_cnt > 0).sum()), "streamed_tasks": int(st_cnt.sum()),
            "digest": hashlib.sha1(np.ascontiguousarray(res_phase, np.int32).tobytes()).hexdigest()[:12]}


def scan():
    """Every layout of the scan, keyed like the fixture (built once per session)."""
    if not _SCAN:
        for name, text in circuits():
            flat = abi.flatten(parseNetlist(text))
            rows_of = row_record_counts(flat)
            for T, rmax in GEOMETRIES:
                for pcr_top, max_tail, rows in PROGRAMS:
                    rec = layout_record(flat, T, rmax, max_tail, pcr_top, rows)
                    if int(rec["meta"][3]) == 0:  # no 16-bit records (the circuit is too large for them): nothing is resident
                        continue
                    rec["rows"] = rows_of + [0] * len(rec["ph_cnt"])
                    _SCAN[f"{name} T={T} rmax={rmax} top={int(pcr_top)} tail={max_tail} rows={int(rows)}"] = rec
    return _SCAN


_SCAN: dict = {}


def test_bench_program_streams_only_its_widest_level():
    """diode_chain(1000) in the packed geometry (512 threads, 4 slots): U_2 (508 tasks, 128 row records) takes the two free
    slot pairs of waves 6 and 7 as row records; only U_0 (2 000 tasks = 512 row records, 16 slot-chunks) stays streamed."""
    flat = abi.flatten(parseNetlist(synth.diode_chain(1000)))
    rec = layout_record(flat, 512, 4, 0, True, True)
    assert [int(x) for x in np.nonzero(rec["st_cnt"])[0]] == [0] and int(rec["st_cnt"][0]) == 2000
    assert rec["res_phase"][6].tolist() == [2, 0xFE, 20, 21] and rec["res_phase"][7].tolist() == [2, 0xFE, 20, 21]
    assert int(rec["meta"][2]) == 0 and int(rec["ph_cnt"].sum()) - rec["streamed_tasks"] == 2719  # (no tail: SpiceyInfo.resident_tasks)


def test_latency_geometry_stays_fully_resident():
    flat = abi.flatten(parseNetlist(synth.diode_chain(1000)))
    for max_tail in (24, 0):
        assert layout_record(flat, 1024, 8, max_tail, True, True)["streamed_tasks"] == 0


def test_layout_invariants_over_the_scan():
    for key, rec in scan().items():
        ph, valid, ph_cnt, st_cnt, meta = rec["res_phase"], rec["res_valid"], rec["ph_cnt"], rec["st_cnt"], rec["meta"]
        nW, rmax = ph.shape
        nL, t0, tn = int(meta[0]), int(meta[1]), int(meta[2])
        resident = np.zeros(len(ph_cnt), np.int64)  # generic records: one task each
        rows_in = np.zeros(len(ph_cnt), np.int64)   # row records: a_ii, y_i and up to two fills of one row, 2..4 tasks each
        for w in range(nW):
            used = int((ph[w] >= 0).sum())
            assert used <= rmax and np.all(ph[w, used:] == -1), key              # compact, no more than rmax slots
            heads = [int(p) for p in ph[w, :used] if p != 0xFE]
            assert heads == sorted(heads), key                                   # phase order inside a wave
            for s in range(used):
                p = int(ph[w, s])
                n_valid = int(valid[s, w * 64:(w + 1) * 64].sum())
                if p == 0xFE:  # a continuation sits directly behind its head, in the same wave; heads are factor phases
                    assert s > 0 and 0 <= ph[w, s - 1] < nL, key
                    continue
                assert 0 <= p < len(ph_cnt) and 1 <= n_valid <= 64, key
                if s + 1 < used and ph[w, s + 1] == 0xFE:
                    rows_in[p] += n_valid
                else:
                    resident[p] += n_valid
        k_merge = 2 * nL - int(meta[5]) if int(meta[4]) > 0 else -1
        for p in range(len(ph_cnt)):
            if t0 <= p < t0 + tn:
                assert resident[p] == 0 and st_cnt[p] == 0, key
            elif rows_in[p] == 0:
                assert resident[p] + st_cnt[p] == ph_cnt[p], (key, p)            # resident + streamed = all tasks
            else:
                assert st_cnt[p] == 0 and rows_in[p] == rec["rows"][p], (key, p)
                assert resident[p] + 2 * rows_in[p] <= ph_cnt[p] <= resident[p] + 4 * rows_in[p], (key, p)
            assert resident[p] + rows_in[p] == 0 or st_cnt[p] == 0, (key, p)     # all resident or all streamed
            assert st_cnt[p] in (0, ph_cnt[p]), (key, p)
            if p == k_merge and resident[p] > 0 and 0 < ph_cnt[p] <= 64:
                assert p in ph[0].tolist() and all(p not in ph[w].tolist() for w in range(1, nW)), key


def test_no_layout_streams_more_than_the_previous_rule_and_changed_ones_stream_fewer_phases():
    with open(GOLDEN) as f:
        parent = json.load(f)
    got = scan()
    assert sorted(parent) == sorted(got)
    fewer = []
    for key, rec in got.items():
        phases, tasks, digest = parent[key]
        assert rec["streamed_phases"] <= phases and rec["streamed_tasks"] <= tasks, key
        if rec["digest"] != digest:
            assert rec["streamed_phases"] < phases, key
            fewer.append(key)
    assert any(k.startswith("diode_chain(1000) T=512 rmax=4 top=1") and k.endswith("rows=1") for k in fewer)


def _first_row_fallback_chain():
    """Smallest chain of the scan whose (512, 4) layout holds row records of a level no wider than the workgroup."""
    for n in range(100, 1201, 50):
        flat = abi.flatten(parseNetlist(synth.diode_chain(n)))
        rec = layout_record(flat, 512, 4, 24, True, True)
        ph = rec["res_phase"]
        for w in range(ph.shape[0]):
            for s in range(1, ph.shape[1]):
                if ph[w, s] == 0xFE and rec["ph_cnt"][int(ph[w, s - 1])] <= 512:
                    return n
    return None


def test_packed_layout_is_bit_identical_to_the_latency_geometry():
    n_small = _first_row_fallback_chain()
    assert n_small is not None
    for n in sorted({1000, n_small}):
        flat, dt, steps, src = synth.chain_batch("diode_chain", n, [1, 2], tran=".tran 1e-6 2e-5")
        assert steps >= 20
        packed = EmulBackend(1, 512, False, 4).run(flat, steps, dt, src)
        latency = EmulBackend(1, 1024, False, 8).run(flat, steps, dt, src)
        assert packed["status"] == 0 and latency["status"] == 0
        for k in ("out_v", "out_i", "iters"):
            assert np.array_equal(packed[k], latency[k]), (n, k)
